"""UperNet-Swin (the HuggingFace provider's default, openmmlab/upernet-swin-small) on the HIP executor against transformers'
UperNetForSemanticSegmentation with a SwinBackbone on the CPU in fp32, seeded random weights (no hub here) — through the C ABI
(flair_upernet_forward).  Tolerances: logits within 1e-3 in fp32, masks by the one parity rule (zero mismatches where the
oracle's top-2 probability gap exceeds 1e-5); bf16 by the logit-error rule of oracle/parity.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL, TINY = (2, 2, 18, 2), (2, 2, 6, 2)
MEANS, STDS = [105.08, 110.87, 101.82], [52.17, 45.38, 44]
# bf16 at 512 x 512, measured: max |dlogit| 1.36e-2 and rms 2.9e-3 of the logit scale (profiles/upernet_parity.json); bounds 3x
BF16_MAX_REL, BF16_RMS_REL = 4.1e-2, 8.6e-3


def seeded_library_model(num_channels=3, num_labels=19, depths=SMALL, seed=2022):
    """transformers' model at the published upernet-swin geometry, random weights; BatchNorm statistics, biases, LayerNorm affine
    parameters and the relative-position tables perturbed so that none of them is at its trivial initial value."""
    from transformers import SwinConfig, UperNetConfig, UperNetForSemanticSegmentation
    torch.manual_seed(seed)
    bc = SwinConfig(embed_dim=96, depths=list(depths), num_heads=[3, 6, 12, 24], window_size=7, mlp_ratio=4.0, qkv_bias=True,
                    layer_norm_eps=1e-5, hidden_act="gelu", num_channels=num_channels, out_features=["stage1", "stage2", "stage3", "stage4"])
    cfg = UperNetConfig(backbone_config=bc, hidden_size=512, pool_scales=[1, 2, 3, 6], use_auxiliary_head=True, auxiliary_in_channels=384,
                        auxiliary_channels=256, auxiliary_num_convs=1, num_labels=num_labels)
    m = UperNetForSemanticSegmentation(cfg).eval()
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=gen))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=gen))
                mod.weight.copy_(0.5 + torch.rand(mod.weight.shape, generator=gen))
        for name, p in m.named_parameters():
            if p.dim() == 1 or "relative_position_bias_table" in name:
                p.add_(0.05 * torch.randn(p.shape, generator=gen))
    return m


@torch.no_grad()
def library_logits(model, x):
    return torch.cat([model(pixel_values=x[i:i + 4]).logits for i in range(0, len(x), 4)])


def _pair(dev, dtype="f32", num_channels=3, depths=SMALL, seed=2022):
    import flair_amd
    ref = seeded_library_model(num_channels, 19, depths, seed)
    hip = flair_amd.UperNetForSemanticSegmentation(num_channels=num_channels, num_labels=19, depths=depths, compute_dtype=dtype)
    hip.load_state_dict(ref.state_dict(), strict=True)
    return ref, hip.to(dev)


@pytest.mark.parametrize("shape,channels,depths", [
    ((1, 128, 128), 3, SMALL),   # stage 4 is 4 x 4: padding, shift and mask inside one window; more PPM bins than pixels
    ((2, 224, 224), 3, SMALL),   # no padding anywhere; stage 4 is exactly one window
    ((1, 256, 384), 3, SMALL),   # a non-square tile
    ((1, 512, 512), 3, SMALL),   # padding at every stage (128 -> 133, 64 -> 70, 32 -> 35, 16 -> 21)
    ((2, 256, 256), 5, TINY),    # swin-tiny through the direct constructor with 5 bands
])
def test_fp32_logits_and_masks_match_the_library(dev, shape, channels, depths):
    """fp32 parity mode: max |dlogit| within 1e-3 of the library (measured: 1.3e-5 .. 1.8e-5 at these shapes, profiles/upernet_parity.json)."""
    from oracle import parity
    ref, hip = _pair(dev, num_channels=channels, depths=depths)
    x = torch.randn(shape[0], channels, shape[1], shape[2], generator=torch.Generator().manual_seed(3))
    want = library_logits(ref, x)
    out = hip(x.to(dev))
    got = out.logits.cpu()
    assert out.loss is None and got.shape == want.shape == (shape[0], 19, shape[1], shape[2]) and got.dtype == torch.float32
    assert torch.equal(hip.forward_full(x.to(dev)).cpu(), got)
    d = float((got - want).abs().max())
    parity.record({"test": f"upernet_swin_fp32_{shape[0]}x{channels}x{shape[1]}x{shape[2]}", "max_abs": d,
                   "logit_scale": float(want.abs().max())})
    assert d < 1e-3, d
    parity.assert_mask_parity(f"upernet_swin_{shape[0]}x{channels}x{shape[1]}x{shape[2]}", want.argmax(1).numpy(), got.argmax(1).numpy(),
                              parity.top2_gap(want.numpy()), logits_ref=want.numpy(), logits_hip=got.numpy())


def test_bf16_mode_tracks_the_library(dev):
    """bf16 throughput mode at 512 x 512: the logit-error rule with bounds 3x the measured error (profiles/upernet_parity.json)."""
    from oracle import parity
    ref, hip = _pair(dev, "bf16")
    x = torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(3))
    want = library_logits(ref, x)
    got = hip(x.to(dev)).logits.cpu()
    scale = float(want.abs().max())
    d = (got - want).abs()
    parity.record({"test": "upernet_swin_bf16_1x3x512x512", "logit_scale": scale, "max_abs": float(d.max()),
                   "rms": float(d.pow(2).mean().sqrt())})
    parity.assert_masks_within_logit_error("upernet_swin_bf16_1x512", want.numpy(), got.numpy(), got.argmax(1).numpy(),
                                           max_rel_dlogit=BF16_MAX_REL, max_rel_rms=BF16_RMS_REL)


def _restatement():
    spec = importlib.util.spec_from_file_location("zone_stitch_restatement", os.path.join(os.path.dirname(__file__), "test_zone_stitch_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _windows_np(raster, cfg, grid):
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


def test_zone_detector_with_upernet_swin_small(dev):
    """zone_detect's window loop with a 3-band UperNet-Swin-small: exact clipping against the sequential CPU restatement
    (oracle/zone_detect.py) fed the library's `.logits`, class_prob, and the three overlap stitching methods against the
    restatement of tests/test_zone_stitch_cpu.py."""
    from flair_amd.zone_detect import ZoneDetector, tile_grid
    from oracle import parity
    from oracle import zone_detect as oz
    ref, hip = _pair(dev)

    class _Library:   # what compare.py calls: model(imgs).logits
        def eval(self):
            return self

        def __call__(self, x):
            return library_logits(ref, x)

    cfg = {"img_pixels_detection": 128, "margin": 32, "output_type": "argmax", "n_classes": 19, "batch_size": 3, "channels": [1, 2, 3],
           "norma_task": [{"norm_type": "custom", "norm_means": MEANS, "norm_stds": STDS}]}
    raster = np.random.default_rng(4).integers(0, 256, size=(3, 168, 200), dtype=np.uint8)
    gap = np.zeros((168, 200))
    want = oz.detect_raster_np(_Library(), raster, cfg, gap_out=gap)
    got = ZoneDetector(hip, cfg).run(torch.from_numpy(raster).to(dev)).cpu().numpy()
    assert got.shape == want.shape == (2, 168, 200)
    parity.assert_mask_parity("zone_detector_upernet_168x200", want[0], got[0], gap)
    assert np.abs(got[1] - want[1]).max() < 1e-4
    cfg2 = dict(cfg, output_type="class_prob", batch_size=5)
    want = oz.detect_raster_np(_Library(), raster, cfg2)
    got = ZoneDetector(hip, cfg2).run(torch.from_numpy(raster).to(dev)).cpu().numpy()
    assert got.shape == (19, 168, 200) and got.dtype == np.uint8
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    R = _restatement()
    S, m, stride = 128, 32, 40
    H, W = raster.shape[1:]
    grid = tile_grid((W, H), S, m, stride)
    lg = library_logits(ref, torch.from_numpy(_windows_np(raster, cfg, grid))).numpy()
    r = torch.from_numpy(raster).to(dev)
    for method in ("average", "average_weights", "max"):
        want, gap = R.stitch_np(lg, grid, H, W, S, m, method)
        got = ZoneDetector(hip, dict(cfg, stitching=method, stride=stride, padding="no-padding")).run(r).cpu().numpy()
        cov = ~np.isinf(gap)
        assert got.shape == want.shape and (got[:, ~cov] == 0).all()
        parity.assert_mask_parity(f"zone_detector_upernet_{method}_168x200", want[0][cov], got[0][cov], gap[cov])
        assert np.abs(got[1][cov] - want[1][cov]).max() < 1e-4, method


def test_factory_and_predict_step(dev):
    """FLAIR_ModelFactory with the reference's HuggingFace keys and 3 channels, then segmentation_task_predict.predict_step:
    the predicted classes against the library's argmax under the parity rule."""
    import flair_amd
    from oracle import parity
    cfg = {"model_framework": {"model_provider": "HuggingFace", "HuggingFace": {"org_model": "openmmlab/upernet-swin-tiny"}},
           "use_metadata": False, "channels": [1, 2, 3], "classes": {i: [1, str(i)] for i in range(1, 20)}}
    ref = seeded_library_model(3, 19, TINY, seed=7)
    f = flair_amd.FLAIR_ModelFactory(cfg)
    f.seg_model.load_state_dict(ref.state_dict(), strict=True)
    f = f.to(dev)
    task = flair_amd.segmentation_task_predict(f, num_classes=19)
    x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(5))
    want = library_logits(ref, x)
    out = task.predict_step({"img": x.to(dev), "id": ["a", "b"]}, 0)
    parity.assert_mask_parity("upernet_predict_step_2x128", want.argmax(1).numpy(), out["preds"].cpu().numpy(), parity.top2_gap(want.numpy()))


def test_cached_weight_layouts_follow_the_parameters(dev):
    """The packed weights, fused q / k / v and folded BatchNorm are reused between forwards (flair_upernet_weights_changed): an
    in-place update of the parameters must be seen by the next forward, and another batch size must not read stale layouts."""
    ref, hip = _pair(dev, depths=TINY, seed=11)
    x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(8))
    cold = hip(x.to(dev)).logits.clone()
    warm = hip(x.to(dev)).logits.clone()
    assert torch.equal(cold, warm)
    ref2 = seeded_library_model(3, 19, TINY, seed=12)
    hip.load_state_dict(ref2.state_dict(), strict=True)                  # in place: same pointers, new contents
    assert float((hip(x.to(dev)).logits.cpu() - library_logits(ref2, x)).abs().max()) < 1e-3
    with torch.no_grad():
        hip.decode_head.classifier.bias.add_(1.0)                        # a single tensor, in place
        ref2.decode_head.classifier.bias.add_(1.0)
    assert float((hip(x.to(dev)).logits.cpu() - library_logits(ref2, x)).abs().max()) < 1e-3
    big = torch.randn(3, 3, 192, 160, generator=torch.Generator().manual_seed(9))   # larger workspace -> new buffer
    assert float((hip(big.to(dev)).logits.cpu() - library_logits(ref2, big)).abs().max()) < 1e-3


def test_contract(dev):
    import flair_amd
    from flair_amd._lib import FlairHipError
    m = flair_amd.UperNetForSemanticSegmentation(num_channels=3, num_labels=19, depths=(1, 1, 1, 1))
    with pytest.raises(FlairHipError):
        m(torch.zeros(1, 3, 128, 128))                  # host tensors are refused: no CPU fallback
    m = m.to(dev)
    for h, w in ((100, 100), (32, 64), (64, 2080)):   # not multiples of 32, below 64, above 2048
        with pytest.raises(RuntimeError, match="multiples of 32 from 64 to 2048"):
            m(torch.zeros(1, 3, h, w, device=dev))
    with pytest.raises(RuntimeError):
        m.train()
    assert m(torch.zeros(2, 3, 64, 64, device=dev)).logits.shape == (2, 19, 64, 64)
    assert m.num_labels == 19
