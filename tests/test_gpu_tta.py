"""Test-time D4 augmentation on the device: the permutation kernel (flair_d4_nchw_f32), the accumulate kernels (flair_tta_accum,
flair_tta_accum_q4) and every surface that takes ``tta=`` (Unet / FLAIR_ModelFactory.predict_classes, SegTrainer.predict,
segmentation_task_predict, ZoneDetector), against the numpy restatement of tests/tta_cases.py.

Bounds: the permutation and the vote counts are exact.  Probabilities: |prob - fp64| <= tol(n) = MAXPROB_ATOL + ((n + 1) / 2 + 1) 2^-24
(tta_cases.tol says why), classes equal wherever the reference's top-2 gap of the mean exceeds 2 tol(n), at most 0.5 % of the pixels
within it.  Model-level references are the fp64 restatement over the cloned logits of the path the package had before
(``eval_logits`` / ``forward`` of the transformed batch), so the new path is never measured against itself.
"""
import numpy as np
import pytest
import torch

import tta_cases as T

pytestmark = pytest.mark.gpu

GUARD = 256
MEANS = [105.08, 110.87, 101.82, 106.38, 53.26]
STDS = [52.17, 45.38, 44, 39.69, 79.3]


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 4: torch.int32}[t.element_size()])


class _Guarded:
    """n elements inside an allocation of n + 2 * GUARD elements filled with ``fill`` (as tests/test_gpu_ce_head_exact.py keeps its outputs)"""

    def __init__(self, dev, n, dtype, fill):
        self.n = n
        self.full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
        self.before = _bits(self.full.cpu().clone())
        self.ptr = self.full.data_ptr() + GUARD * self.full.element_size()

    def read(self, what):
        after = self.full.cpu()
        a = _bits(after)
        assert torch.equal(a[:GUARD], self.before[:GUARD]), f"{what}: written before the buffer"
        assert torch.equal(a[GUARD + self.n:], self.before[GUARD + self.n:]), f"{what}: written behind the buffer"
        return after[GUARD:GUARD + self.n]


def _lib():
    from flair_amd import _lib as L
    return L, L.lib()


def _run_passes(dev, logits, codes, shape, quarter=False, want_prob=True):
    """The raw C calls over guarded buffers, acc NaN-filled: (preds u8, prob f32, acc bits after pass n-2, acc bits after pass n-1)"""
    L, lib = _lib()
    B, C, H, W = shape
    n = len(codes)
    acc = _Guarded(dev, B * C * H * W, torch.float32, float("nan"))
    preds = _Guarded(dev, B * H * W, torch.uint8, 201)
    prob = _Guarded(dev, B * H * W, torch.float32, -5.0)
    fn = lib.flair_tta_accum_q4 if quarter else lib.flair_tta_accum
    acc_before = None
    for k, (lg, code) in enumerate(zip(logits, codes)):
        last = k == n - 1
        if last:
            acc_before = _bits(acc.read("acc")).clone()
        lgd = lg.to(dev).contiguous() if torch.is_tensor(lg) else torch.from_numpy(lg).to(dev)
        rc = fn(L.ptr(lgd), B, C, H, W, code, int(k == 0), acc.ptr, preds.ptr if last else None, prob.ptr if last and want_prob else None,
                n, L.stream())
        assert rc == 0, (rc, k, code)
        torch.cuda.synchronize()
    return (preds.read("preds").view(B, H, W).numpy(), prob.read("prob").view(B, H, W).numpy(), acc_before, _bits(acc.read("acc")))


# ------------------------------------------------------------------------------------------------------ d4 kernel, bit-exact

@pytest.mark.parametrize("shape,codes", [((2, 3, 8, 8), T.ALL16), ((1, 5, 64, 64), T.ALL16), ((3, 1, 32, 96), T.EVEN_K),
                                         ((1, 2, 5, 7), T.EVEN_K), ((1, 2, 33, 33), T.ALL16)],
                         ids=["2x3x8x8", "1x5x64x64", "3x1x32x96", "1x2x5x7", "1x2x33x33"])
def test_d4_kernel_is_the_permutation(dev, shape, codes):
    """every code; 64 x 64 spans four 32 x 32 tiles per plane, 5 x 7 and 33 x 33 end inside a tile"""
    from flair_amd import ops
    x = np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    for code in codes:
        got = ops.d4_transform(xd, code)
        assert got.shape == xd.shape and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy().view(np.int32), T.d4_np(x, code).view(np.int32)), code
    assert torch.equal(xd.cpu(), torch.from_numpy(x))   # out of place


def test_d4_kernel_refusals_launch_nothing(dev):
    from flair_amd import ops
    L, lib = _lib()
    x = torch.ones(1, 2, 32, 96, device=dev)
    out = _Guarded(dev, x.numel(), torch.float32, 7.0)
    st = L.stream()
    for code in (4, 5, 6, 7, 12, 13, 14, 15):
        assert lib.flair_d4_nchw_f32(L.ptr(x), out.ptr, 1, 2, 32, 96, code, st) == -19
    for code in (-1, 16, 255):
        assert lib.flair_d4_nchw_f32(L.ptr(x), out.ptr, 1, 2, 32, 96, code, st) == -2
    assert lib.flair_d4_nchw_f32(None, out.ptr, 1, 2, 32, 96, 0, st) == -1
    assert lib.flair_d4_nchw_f32(L.ptr(x), None, 1, 2, 32, 96, 0, st) == -1
    assert lib.flair_d4_nchw_f32(L.ptr(x), L.ptr(x), 1, 2, 32, 96, 0, st) == -1          # in place
    assert lib.flair_d4_nchw_f32(L.ptr(x), out.ptr, 0, 2, 32, 96, 0, st) == -2
    torch.cuda.synchronize()
    assert (out.read("d4 refusals") == 7).all()
    assert lib.flair_strerror(-19).decode().startswith("D4 transform code")
    with pytest.raises(ValueError, match="square"):
        ops.d4_transform(x, 4)
    with pytest.raises(ValueError):
        ops.d4_transform(x, 16)


def test_d4_kernel_equals_the_feed_kernels_augmentation(dev):
    """flair_feed_tiles with d4 = code and norm 'without' == d4_transform(flair_feed_tiles without d4), bit for bit, for all 16 codes:
    the new kernel against the feed's reference-pinned definition"""
    from flair_amd import ops
    from flair_amd.data_feed import TileFeed
    B = 16
    img = torch.from_numpy(np.random.default_rng(9).integers(0, 256, size=(B, 5, 32, 32), dtype=np.uint8)).to(dev)
    feed = TileFeed(channels=(1, 2, 3, 4, 5), norm_type="without")
    plain = feed(img)["img"]
    aug = feed(img, d4=torch.arange(16, dtype=torch.uint8, device=dev))["img"]
    for code in T.ALL16:
        assert torch.equal(_bits(aug[code:code + 1]), _bits(ops.d4_transform(plain[code:code + 1].contiguous(), code))), code


# --------------------------------------------------------------------------------------------------- accumulate, exact votes

@pytest.mark.parametrize("hw", [(2, 8, 8), (1, 64, 64), (1, 32, 64)], ids=["2x8x8", "1x64x64", "1x32x64"])
@pytest.mark.parametrize("C", T.CLASSES)
def test_accumulate_counts_votes_exactly(dev, C, hw):
    """one-hot softmaxes (+-120 logits): prob == votes / n bit for bit, preds == the lowest class with most votes (ties are frequent);
    acc starts as NaN, every output sits in a guarded buffer, and the last pass leaves acc as the pass before left it"""
    B, H, W = hw
    for n in T.PASSES:
        codes = T.vote_codes(n, 100 * C + n)
        if H != W:
            codes = [c & 0b1011 for c in codes]
        logits, want_preds, want_prob = T.vote_case(B, C, H, W, codes, 1000 * n + C + H)
        preds, prob, acc_before, acc_after = _run_passes(dev, logits, codes, (B, C, H, W))
        assert np.array_equal(preds, want_preds), (n, codes)
        assert np.array_equal(prob.view(np.int32), want_prob.view(np.int32)), (n, codes)
        assert torch.equal(acc_before, acc_after), (n, "the last pass wrote acc")
        nan_bits = _bits(torch.full((1,), float("nan")))[0]
        if n == 1:
            assert (acc_after == nan_bits).all()        # first and last: acc never touched
        else:
            assert not (acc_after == nan_bits).any()    # `first` stored over the NaNs, nothing was added to one


def test_accumulate_without_prob_and_without_acc(dev):
    L, lib = _lib()
    logits, want_preds, _ = T.vote_case(2, 13, 8, 8, [6], 3)
    preds, prob, _, _ = _run_passes(dev, logits, [6], (2, 13, 8, 8), want_prob=False)
    assert np.array_equal(preds, want_preds) and (prob == -5.0).all()
    p = torch.full((2, 8, 8), 9, dtype=torch.uint8, device=dev)
    assert lib.flair_tta_accum(L.ptr(torch.from_numpy(logits[0]).to(dev)), 2, 13, 8, 8, 6, 1, None, L.ptr(p), None, 1, L.stream()) == 0
    assert np.array_equal(p.cpu().numpy(), want_preds)


def test_accumulate_refusals_launch_nothing(dev):
    L, lib = _lib()
    lg = torch.ones(1, 33, 32, 64, device=dev)
    acc = torch.full((1, 33, 32, 64), 7.0, device=dev)
    preds = torch.full((1, 32, 64), 7, dtype=torch.uint8, device=dev)
    prob = torch.full((1, 32, 64), 7.0, device=dev)
    st, p = L.stream(), L.ptr
    for fn in (lib.flair_tta_accum, lib.flair_tta_accum_q4):
        assert fn(None, 1, 13, 32, 32, 0, 1, p(acc), p(preds), p(prob), 1, st) == -1
        assert fn(p(lg), 1, 13, 32, 32, 0, 1, p(acc), None, p(prob), 2, st) == -1              # prob without preds
        assert fn(p(lg), 1, 13, 32, 32, 0, 0, None, p(preds), p(prob), 2, st) == -1             # a later pass needs acc
        assert fn(p(lg), 1, 13, 32, 32, 0, 1, None, None, None, 2, st) == -1                    # a first pass that is not last, too
        for C in (0, 33):
            assert fn(p(lg), 1, C, 32, 32, 0, 1, p(acc), p(preds), p(prob), 1, st) == -2
        for n in (0, 17):
            assert fn(p(lg), 1, 13, 32, 32, 0, 1, p(acc), p(preds), p(prob), n, st) == -2
        for code in (-1, 16):
            assert fn(p(lg), 1, 13, 32, 32, code, 1, p(acc), p(preds), p(prob), 1, st) == -2
        assert fn(p(lg), 1, 13, 32, 64, 4, 1, p(acc), p(preds), p(prob), 1, st) == -19             # odd k, H != W
    assert lib.flair_tta_accum_q4(p(lg), 1, 13, 32, 64, 0, 1, p(acc), p(preds), p(prob), 1, st) == -2   # quarter source: square tiles
    assert lib.flair_tta_accum_q4(p(lg), 1, 13, 30, 30, 0, 1, p(acc), p(preds), p(prob), 1, st) == -2   # and a side divisible by 4
    torch.cuda.synchronize()
    assert (acc == 7).all() and (preds == 7).all() and (prob == 7).all()


# ------------------------------------------------------------------------------------------------------ accumulate, numeric

@pytest.mark.parametrize("codes,seed", [(T.D4, 2), ([0, 1, 2], 148)], ids=["d4", "0-1-2"])
def test_accumulate_random_logits_vs_fp64(dev, codes, seed):
    """logits 8 * randn on (2, 13, 64, 64), an independent draw per pass.  Seeds: with the eight d4 codes seed 2 leaves no pixel within
    2 tol(8) of a tie.  With [0, 1, 2] no seed of 0..299 does: at this logit scale most softmaxes are one-hot to fp32 precision, and
    three passes with three different winners tie to within 1e-7; seed 148 has the fewest such pixels (4 of 8 192, 0.05 %), the 0.5 %
    cap stands."""
    rng = np.random.default_rng(seed)
    shape = (2, 13, 64, 64)
    logits = [(8 * rng.standard_normal(shape)).astype(np.float32) for _ in codes]
    ref = T.ensemble_ref(logits, codes)
    preds, prob, _, _ = _run_passes(dev, logits, codes, shape)
    fig = T.check_against_ref(f"tta_accum_random_{len(codes)}", preds, prob, ref, len(codes))
    if len(codes) == 8:
        assert fig["excluded"] == 0.0
    # the Python binding drives the same passes
    from flair_amd import tta
    it = iter(logits)
    p2, q2 = tta.tta_predict(lambda t: torch.from_numpy(next(it)).to(dev), torch.zeros(2, 1, 64, 64, device=dev), codes, want_prob=True)
    assert np.array_equal(p2.cpu().numpy(), preds) and np.array_equal(q2.cpu().numpy().view(np.int32), prob.view(np.int32))


# ------------------------------------------------------------------------------------------------------------ quarter source

@pytest.mark.parametrize("C", [13, 19])
@pytest.mark.parametrize("S", [16, 64])
def test_accumulate_q4_equals_full_resolution_on_exact_inputs(dev, S, C):
    """integer quarter logits in [-8, 8] (tests/test_gpu_zone_quarter.py's family: every x4-interpolated value is a multiple of 1/64,
    exact in fp32): flair_tta_accum_q4 == flair_tta_accum fed the x4 bilinear kernel's output, bit for bit"""
    from flair_amd import ops
    for codes in (T.D4, [7, 0, 14]):
        rng = np.random.default_rng(S + C + len(codes))
        lq = [torch.from_numpy(rng.integers(-8, 9, size=(3, C, S // 4, S // 4)).astype(np.float32)).to(dev) for _ in codes]
        lf = [ops.sf_bilinear_nchw_f32(q, S, S) for q in lq]
        pq, qq, _, _ = _run_passes(dev, lq, codes, (3, C, S, S), quarter=True)
        pf, qf, _, _ = _run_passes(dev, lf, codes, (3, C, S, S))
        assert np.array_equal(pq, pf) and np.array_equal(qq.view(np.int32), qf.view(np.int32)), codes
        assert len(np.unique(pq)) > 1


# ---------------------------------------------------------------------------------------------------------- U-Net end to end

def _unet(dev, dtype, classes=13):
    import flair_amd
    from oracle import unet_resnet34 as om
    ref = om.seeded_model(5, classes, 2022)
    hip = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=classes, compute_dtype=dtype)
    hip.load_state_dict(ref.state_dict(), strict=True)
    return hip.to(dev).eval()


def _pass_logits(logits_fn, x, codes):
    from flair_amd import ops
    return [logits_fn(ops.d4_transform(x, code)).clone().cpu().numpy() for code in codes]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_unet_predict_classes_tta(dev, dtype):
    hip = _unet(dev, dtype)
    x = torch.randn(2, 5, 64, 64, generator=torch.Generator().manual_seed(5)).to(dev)
    plain, plain_prob = hip.predict_classes(x, want_prob=True)
    for spec in ("d4", "flips", [0, 1, 2]):
        codes = T.D4 if spec == "d4" else T.FLIPS if spec == "flips" else spec
        ref = T.ensemble_ref(_pass_logits(hip.eval_logits, x, codes), codes)
        preds, prob = hip.predict_classes(x, want_prob=True, tta=spec)
        assert preds.dtype == torch.uint8 and preds.shape == (2, 64, 64) and prob.dtype == torch.float32
        T.check_against_ref(f"unet_{dtype}_tta_{spec}", preds.cpu().numpy(), prob.cpu().numpy(), ref, len(codes))
        assert torch.equal(hip.predict_classes(x, tta=spec), preds)          # without prob: the same classes
        if spec == "d4":
            changed = float((preds != plain).float().mean())
            print(f"unet_{dtype}: tta='d4' changes {changed:.1%} of the pixels")
            assert changed >= 0.01
    # one identity pass is the plain prediction.  Off near-ties: the plain path takes its argmax in the head convolution's epilogue,
    # the ensemble from the fp32 NCHW logits; in bf16 mode those may have gone through a bf16 store, which moves a logit l by at
    # most 2^-8 |l|, so two logits closer than 2^-7 max|l| may swap.  fp32 mode: the probability gap rule alone.
    lg = hip.eval_logits(x).clone().cpu().double()
    top = lg.topk(2, dim=1).values
    sure = T.ensemble_ref([lg.numpy()], [0])[2] > 2 * T.tol(1)
    if dtype == "bf16":
        sure &= ((top[:, 0] - top[:, 1]) > 2.0 ** -7 * top.abs().amax(dim=1)).numpy()
    assert sure.mean() > (0.995 if dtype == "f32" else 0.9), sure.mean()
    one, one_prob = hip.predict_classes(x, want_prob=True, tta=[0])
    assert np.array_equal(one.cpu().numpy()[sure], plain.cpu().numpy()[sure])
    if dtype == "f32":
        assert float((one_prob - plain_prob).abs().max()) <= 2 * T.MAXPROB_ATOL
    with pytest.raises(ValueError):
        hip.predict_classes(x, tta="D4")
    with pytest.raises(ValueError, match="square"):
        hip.predict_classes(torch.zeros(1, 5, 64, 96, device=dev), tta="d4")
    # off: the very tensors of the plain call
    for off in (None, "none", []):
        p0, q0 = hip.predict_classes(x, want_prob=True, tta=off)
        assert torch.equal(p0, plain) and torch.equal(_bits(q0), _bits(plain_prob))


CLASSES13 = {i: [1, f"class {i}"] for i in range(1, 14)}


def _factory(dev, use_metadata):
    import flair_amd
    from oracle import unet_resnet34 as om
    cfg = {"model_framework": {"model_provider": "SegmentationModelsPytorch",
                               "SegmentationModelsPytorch": {"encoder_decoder": "resnet34_unet", "encoder_weights": None}},
           "use_metadata": use_metadata, "channels": [1, 2, 3, 4, 5], "classes": CLASSES13}
    state = torch.random.get_rng_state()
    torch.manual_seed(2023)
    try:
        model = flair_amd.FLAIR_ModelFactory(cfg, compute_dtype="f32")
    finally:
        torch.random.set_rng_state(state)
    model.seg_model.load_state_dict(om.seeded_model(5, 13, 2022).state_dict(), strict=True)
    return model.to(dev).eval()


def test_metadata_goes_unchanged_to_every_pass(dev):
    """B = 1 at 512 x 512 (the only size the metadata branch takes): the factory and SegTrainer.predict.
    The tile: 0.2 * (a 16 x 16 normal field resized to 512 x 512 + 0.5 * noise).  On a unit-variance noise tile this seeded model's
    logits reach +-200, every softmax is one-hot and the four flips split 2 : 2 on 1.6 % of the pixels (CPU oracle), exact ties the
    0.5 % cap has no room for; at this scale the logits stay within +-33 and the oracle leaves no pixel within 2 tol(4) of a tie."""
    import flair_amd
    model = _factory(dev, True)
    g = torch.Generator().manual_seed(8)
    lo = torch.randn(1, 5, 16, 16, generator=g)
    x = 0.2 * (torch.nn.functional.interpolate(lo, size=(512, 512), mode="bilinear", align_corners=False)
               + 0.5 * torch.randn(1, 5, 512, 512, generator=g))
    x, mtd = x.to(dev), torch.rand(1, 45, generator=g).to(dev)
    with torch.no_grad():
        ref = T.ensemble_ref(_pass_logits(lambda t: model(t, mtd), x, T.FLIPS), T.FLIPS)
        without = T.ensemble_ref(_pass_logits(model.seg_model.eval_logits, x, T.FLIPS), T.FLIPS)
    assert np.abs(ref[1] - without[1]).max() > 1e-3     # the metadata matters
    preds, prob = model.predict_classes(x, mtd, want_prob=True, tta="flips")
    T.check_against_ref("factory_metadata_tta_flips", preds.cpu().numpy(), prob.cpu().numpy(), ref, 4)
    tr = flair_amd.SegTrainer(model.seg_model, lr=0.0, metadata_encoder=model.enc)
    assert torch.equal(tr.predict(x, mtd, tta="flips"), preds)
    assert torch.equal(tr.predict(x, mtd, tta="none"), model.predict_classes(x, mtd))
    with pytest.raises(ValueError, match="metadata"):
        model.predict_classes(x, tta="flips")


def test_predict_step_hands_int64_classes_to_the_writer(dev):
    import flair_amd
    from flair_amd import tasks_utils
    model = _factory(dev, False)
    x = torch.randn(2, 5, 64, 64, generator=torch.Generator().manual_seed(5)).to(dev)
    want = model.predict_classes(x, tta="flips")
    assert torch.equal(want, model.seg_model.predict_classes(x, tta=[0, 1, 2, 3]))
    task = flair_amd.segmentation_task_predict(model, num_classes=13, tta="flips")
    out = task.predict_step({"img": x, "id": ["a", "b"]}, 0)
    assert out["preds"].dtype == torch.int64 and torch.equal(out["preds"], want.to(torch.int64))
    plain = flair_amd.segmentation_task_predict(model, num_classes=13).predict_step({"img": x}, 0)["preds"]
    assert plain.dtype == torch.int64 and torch.equal(plain, model.predict_classes(x).to(torch.int64)) and not torch.equal(plain, out["preds"])
    assert flair_amd.SegTrainer(model.seg_model, lr=0.0).predict(x, tta="flips").equal(want)
    # the config key reaches the predict module (and only it)
    cfg = {"model_framework": {"model_provider": "SegmentationModelsPytorch",
                               "SegmentationModelsPytorch": {"encoder_decoder": "resnet34_unet", "encoder_weights": None}},
           "use_metadata": False, "channels": [1, 2, 3, 4, 5], "classes": CLASSES13, "tta": "d4"}
    assert tasks_utils.get_segmentation_module(cfg, stage="predict").tta == T.D4
    assert tasks_utils.get_segmentation_module({**cfg, "tta": "none"}, stage="predict").tta is None
    with pytest.raises(ValueError):
        tasks_utils.get_segmentation_module({**cfg, "tta": "all"}, stage="predict")


# ------------------------------------------------------------------------------------------------------ HuggingFace provider

def _spread_logits(segformer):
    """A SegFormer as initialised (normal(0, 0.02) weights) gives logits within a few 1e-3 of each other: all 19 mean probabilities
    sit at 1 / 19 and 0.4 - 0.6 % of the pixels have a top-2 gap under 2 tol(4) (measured; the 0.5 % cap has no room for that).  A
    classifier 50 times larger spreads them; the test is about the ensemble, not about these weights."""
    if type(segformer).__name__.startswith("Segformer"):
        with torch.no_grad():
            segformer.decode_head.classifier.weight.mul_(50.0)


def _hf_factory(dev, org, channels, seed, **extra):
    import flair_amd
    cfg = {"model_framework": {"model_provider": "HuggingFace", "HuggingFace": {"org_model": org, **extra}},
           "use_metadata": False, "channels": channels, "classes": {i: [1, str(i)] for i in range(1, 20)}}
    torch.manual_seed(seed)
    f = flair_amd.FLAIR_ModelFactory(cfg, compute_dtype="f32")
    _spread_logits(f.seg_model)
    return f.to(dev).eval()


@pytest.mark.parametrize("which", ["segformer", "upernet"])
def test_huggingface_provider_tta_flips(dev, which):
    """SegFormer (depths 1-1-1-1, decoder 256) at 128 x 128: the factory's logits are quarter-size (quirk Q11) and so is the result;
    UperNet-Swin-tiny: full size"""
    if which == "segformer":
        f = _hf_factory(dev, "nvidia/mit-b1", [1, 2, 3, 4, 5], 7, depths=[1, 1, 1, 1], decoder_hidden_size=256)
        n_ch, side = 5, 32
    else:
        f = _hf_factory(dev, "openmmlab/upernet-swin-tiny", [1, 2, 3], 11)
        n_ch, side = 3, 128
    x = torch.randn(2, n_ch, 128, 128, generator=torch.Generator().manual_seed(5)).to(dev)
    with torch.no_grad():
        ref = T.ensemble_ref(_pass_logits(f.forward, x, T.FLIPS), T.FLIPS)
    preds, prob = f.predict_classes(x, want_prob=True, tta="flips")
    assert preds.shape == (2, side, side) and preds.dtype == torch.uint8
    T.check_against_ref(f"factory_{which}_tta_flips", preds.cpu().numpy(), prob.cpu().numpy(), ref, 4)
    assert torch.equal(f.predict_classes(x, tta="flips"), preds)


# --------------------------------------------------------------------------------------------------------------- zone_detect

def _zcfg(C, **kw):
    c = {"img_pixels_detection": 64, "margin": 8, "output_type": "argmax", "n_classes": C, "batch_size": 5,
         "channels": [1, 2, 3, 4, 5], "norma_task": [{"norm_type": "custom", "norm_means": MEANS, "norm_stds": STDS}],
         "classes": {c: [1, f"class {c}"] for c in range(1, C + 1)}}
    c.update(kw)
    return c


def _gather(det, r, tiles):
    L, lib = _lib()
    from flair_amd.data_feed import NORM_CODES
    bands, Hr, Wr = r.shape
    n = len(det.channels)
    imgs = torch.empty(len(tiles), n, det.S, det.S, dtype=torch.float32, device=r.device)
    L.check(lib.flair_gather_tiles(L.ptr(r), bands, Hr, Wr, L.ptr(tiles), len(tiles), det.S, det._ch, n, NORM_CODES[det.norm_type],
                                   det._means, det._stds, L.ptr(imgs), L.stream()))
    return imgs


def _replay(det, r, predict, stitching, truth=None):
    """numpy: ``predict(windows) -> (preds, prob)`` per batch of the run's own windows, painted in job order.  exact-clipping: each
    window's owned rectangle; max: its margin-cropped core, kept unless the held probability is strictly greater.  With ``truth``
    also each window's confusion matrix over its core (exact-clipping: of its own classes; max: of the finished raster)."""
    from flair_amd.zone_detect import tile_grid
    _, Hr, Wr = r.shape
    S, m, C = det.S, det.margin, det.n_classes
    grid = tile_grid((Wr, Hr), S, m, det.stride)
    tiles = torch.from_numpy(grid).to(r.device)
    out = np.zeros((2, Hr, Wr), np.float32)
    own = []
    for b0 in range(0, len(grid), det.batch_size):
        p, q = predict(_gather(det, r, tiles[b0:b0 + det.batch_size].contiguous()))
        p, q = p.cpu().numpy(), q.cpu().numpy()
        for b, (x0, y0, wx0, wx1, wy0, wy1) in enumerate(grid[b0:b0 + det.batch_size]):
            own.append(p[b])
            if stitching == "exact-clipping":
                out[0, wy0:wy1, wx0:wx1] = p[b][wy0 - y0:wy1 - y0, wx0 - x0:wx1 - x0]
                out[1, wy0:wy1, wx0:wx1] = q[b][wy0 - y0:wy1 - y0, wx0 - x0:wx1 - x0]
                continue
            ya, yb, xa, xb = max(y0 + m, 0), min(y0 + S - m, Hr), max(x0 + m, 0), min(x0 + S - m, Wr)
            pw, qw = p[b][ya - y0:yb - y0, xa - x0:xb - x0], q[b][ya - y0:yb - y0, xa - x0:xb - x0]
            keep = out[1, ya:yb, xa:xb] > qw
            out[0, ya:yb, xa:xb] = np.where(keep, out[0, ya:yb, xa:xb], pw)
            out[1, ya:yb, xa:xb] = np.where(keep, out[1, ya:yb, xa:xb], qw)
    cms = None
    if truth is not None:
        cms = np.zeros((len(grid), C, C), np.int64)
        for b, (x0, y0) in enumerate(grid[:, :2]):
            ya, yb, xa, xb = max(y0 + m, 0), min(y0 + S - m, Hr), max(x0 + m, 0), min(x0 + S - m, Wr)
            t = (truth[ya:yb, xa:xb].astype(np.uint8) - np.uint8(1)).astype(np.int64)
            pr = (own[b][ya - y0:yb - y0, xa - x0:xb - x0] if stitching == "exact-clipping" else out[0, ya:yb, xa:xb]).astype(np.int64)
            ok = (t < C) & (pr < C)
            np.add.at(cms[b], (t[ok], pr[ok]), 1)
    return out, cms


@pytest.fixture(scope="module")
def zone_unet(dev):
    return _unet(dev, "f32")


@pytest.fixture(scope="module")
def zone_raster(dev):
    rng = np.random.default_rng(31)
    return (torch.from_numpy(rng.integers(0, 256, size=(5, 150, 170), dtype=np.uint8)).to(dev),
            rng.integers(0, 15, size=(150, 170)).astype(np.uint8))


@pytest.mark.parametrize("stride", [48, 24])
@pytest.mark.parametrize("stitching", ["exact-clipping", "max"])
def test_zone_detector_tta_unet(dev, zone_unet, zone_raster, stitching, stride):
    from flair_amd import tta
    from flair_amd.zone_detect import ZoneDetector
    r, truth = zone_raster
    td = torch.from_numpy(truth).to(dev)
    for spec in ("flips", "d4"):
        det = ZoneDetector(zone_unet, _zcfg(13, stitching=stitching, stride=stride, padding="no-padding", tta=spec))
        got = det.run(r, td)
        codes = tta.tta_codes(spec)
        want, cms = _replay(det, r, lambda w: tta.tta_predict(zone_unet.eval_logits, w, codes, want_prob=True), stitching, truth)
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), spec
        assert np.array_equal(det.window_confmats.cpu().numpy(), cms) and cms.sum() > 0, spec
    # without the key, and with "none": the raster of the plain path, bit for bit
    plain = ZoneDetector(zone_unet, _zcfg(13, stitching=stitching, stride=stride, padding="no-padding"))
    none = ZoneDetector(zone_unet, _zcfg(13, stitching=stitching, stride=stride, padding="no-padding", tta="none"))
    assert plain.tta is None and none.tta is None
    out = plain.run(r)
    want, _ = _replay(plain, r, lambda w: zone_unet.predict_classes(w, want_prob=True), stitching)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    assert torch.equal(_bits(none.run(r)), _bits(out))
    assert not torch.equal(out[0], got[0])    # and the ensemble's differs from it


def test_zone_detector_tta_segformer_quarter_path(dev, monkeypatch, zone_raster):
    """SegFormer takes tiles of 128 and up: S = 128, margin 8, stride 48 on the same raster, quarter logits into flair_tta_accum_q4"""
    import flair_amd
    from flair_amd import tta
    from flair_amd.zone_detect import ZoneDetector
    torch.manual_seed(7)
    model = flair_amd.SegformerForSemanticSegmentation(num_channels=5, num_labels=19, depths=(1, 1, 1, 1), decoder_hidden_size=256,
                                                       compute_dtype="f32")
    _spread_logits(model)
    model = model.to(dev).eval()
    r, truth = zone_raster
    monkeypatch.setenv("FLAIR_ZD_QUARTER", "1")
    calls = {"full": 0}
    real_full = model.forward_full

    def forward_full(x):
        calls["full"] += 1
        return real_full(x)

    monkeypatch.setattr(model, "forward_full", forward_full, raising=False)
    for stitching in ("exact-clipping", "max"):
        det = ZoneDetector(model, _zcfg(19, img_pixels_detection=128, stitching=stitching, stride=48, padding="no-padding", batch_size=3,
                                        tta="flips"))
        assert det.quarter
        got = det.run(r, torch.from_numpy(truth).to(dev))
        want, cms = _replay(det, r, lambda w: tta.tta_predict(model.forward_quarter, w, T.FLIPS, want_prob=True, quarter=True), stitching,
                            truth)
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), stitching
        assert np.array_equal(det.window_confmats.cpu().numpy(), cms), stitching
    assert calls["full"] == 0
    # the quarter accumulate against the x4 pass and the full-resolution accumulate, under the probability bound
    from flair_amd import ops
    w = torch.randn(2, 5, 128, 128, generator=torch.Generator().manual_seed(3)).to(dev)
    ref = T.ensemble_ref([ops.sf_bilinear_nchw_f32(model.forward_quarter(ops.d4_transform(w, c)), 128, 128).cpu().numpy() for c in T.FLIPS],
                         T.FLIPS)
    p, q = tta.tta_predict(model.forward_quarter, w, T.FLIPS, want_prob=True, quarter=True)
    assert p.shape == (2, 128, 128)
    T.check_against_ref("segformer_quarter_tta_flips", p.cpu().numpy(), q.cpu().numpy(), ref, 4)


def test_zone_detector_tta_refuses_per_class_outputs(dev, zone_unet):
    from flair_amd.zone_detect import ZoneDetector
    for kw in ({"output_type": "class_prob"}, {"stitching": "average", "stride": 24}, {"stitching": "average_weights", "stride": 24},
               {"output_type": "class_prob", "stitching": "max", "stride": 24}):
        with pytest.raises(ValueError, match="tta"):
            ZoneDetector(zone_unet, _zcfg(13, tta="flips", **kw))
        ZoneDetector(zone_unet, _zcfg(13, **kw))             # the same config without tta stands
        ZoneDetector(zone_unet, _zcfg(13, tta="none", **kw))
    with pytest.raises(ValueError):
        ZoneDetector(zone_unet, _zcfg(13, tta="rot"))
