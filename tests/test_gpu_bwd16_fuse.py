"""The fused backward of the 16-channel 3x3 tail convolutions (csrc/bwd_halo16.hip: data gradient + BatchNorm-backward sums of the
upstream unit + weight gradient (+ bias gradient) in one kernel; tune key FLAIR_BWD16_FUSE, grid FLAIR_BWD16_WGS).

1. Whole step, fused against separate: SegTrainer.train_step, bf16, 13 classes, two steps, at B=2 64x64 (32 full-resolution tiles)
   and B=1 96x96 (36 tiles, one of them without a border; no multiple of either grid).  FLAIR_BWD16_WGS = FLAIR_WGH_WGS = g pins
   the fused kernel's and the separate weight gradient's grids to g = 3 and 5 workgroups, so a workgroup walks 6 to 12 tiles through
   both register slots, and 7 / 11 / 8 tiles end a walk on the even slot.  FLAIR_HALO_P_WGS is set to g as well; it is a per-CU
   cap (256 x g workgroups), so at these sizes the separate data gradient runs one tile per workgroup and leaves one partial column
   per tile — the fused kernel keeps exactly that layout of the BatchNorm-backward partials (Bwd16Args::bnr_cols), which is what
   makes the two paths bit-identical here.  grads, loss, parameters and buffers: torch.equal.
2. Fallbacks: 19 classes (head rows 32 wide) keep the head on the separate kernels, fp32 keeps both layers there; checked through
   the launch profile, where case 1 shows both fused kernels and none of the launches they replace.  The shape condition (H % 8,
   W % 32) cannot fail inside the network, which takes multiples of 32 only: it is checked at the operator entry (-2).
3. Exact arithmetic: small-integer gradients, activations, weights and coefficients, every sum exact in fp32 and every stored value
   exact in bf16 (asserted on the reference): dx, the BatchNorm-backward sums, dW and the head's dbias equal the fp64 torch
   reference whatever the grid (1, 3, the default), both flavours, at 16x64 (B=2) and 24x96.
4. Workspace: flair_unet_workspace_bytes(training = 2), the dry run of the whole-model training step as it runs, is smaller with
   the fused path than without it by exactly the dy tensor of decoder block 4's second convolution (the head has no dy), and two
   steps on a workspace of exactly that size pass and give the bits of the steps on the default workspace.  (training = 1 stays
   the bound of the split sequence, which never takes the fused path and still needs dy.)
5. Default grids above the grid size: B=4 256x512 (2048 tiles on the separate weight gradient's grid, 768 workgroups where three fit
   per CU: walks of two and three tiles, the BatchNorm-backward partials carried across a walk, one column per workgroup), no pins:
   the fused kernels are in the step — a fallback on disagreeing occupancy answers would fail here — and fused = separate bit for
   bit."""
import functools
import os
import re

import pytest
import torch

import exact_cases as E
import launch_helpers as LH

pytestmark = pytest.mark.gpu

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flair-1_amd", "csrc", "bwd_halo16.h")
FUSE_DEFAULT = int(re.search(r"FLAIR_BWD16_FUSE_DEFAULT = (\d+)", open(_HDR).read()).group(1))
DEFAULTS = {"FLAIR_BWD16_FUSE": FUSE_DEFAULT, "FLAIR_BWD16_WGS": 0, "FLAIR_WGH_WGS": 0, "FLAIR_HALO_P_WGS": 0}
FUSED = ("bwd16_fused_head_bf16", "bwd16_fused_unit_bf16")


def _tuned(**pairs):
    return LH.tuned(pairs.items(), DEFAULTS)


_profiled = functools.partial(LH.profiled, slots=2048)   # every kernel of whole training steps


@pytest.fixture(scope="module")
def states():
    """seeded reference weights per (classes): built once, loaded into every model of this module, never modified"""
    from oracle import unet_resnet34 as om
    built = {}

    def state(classes):
        if classes not in built:
            built[classes] = om.seeded_model(5, classes, 31).state_dict()
        return built[classes]

    return state


STEPS = 2


def _steps(dev, state, classes, shape, dtype, prepare=None):
    """STEPS training steps of a fresh model; what they leave, and the launches of all of them"""
    import flair_amd
    m = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=classes, compute_dtype=dtype)
    m.load_state_dict(state(classes), strict=True)
    m = m.to(dev).train()
    if prepare:
        prepare(m)
    w = torch.linspace(0.5, 2, classes)
    tr = flair_amd.SegTrainer(m, lr=0.05, class_weight=w)
    g = torch.Generator().manual_seed(shape[2])
    out = {"loss": [], "grads": []}

    def run():
        for _ in range(STEPS):
            x = torch.randn(*shape, generator=g).to(dev)
            lab = torch.randint(0, classes, (shape[0], shape[2], shape[3]), generator=g).to(torch.uint8).to(dev)
            out["loss"].append(tr.train_step(x, lab).clone())
            out["grads"].append(tr.grads.clone())

    _, ran = _profiled(run)
    torch.cuda.synchronize()
    out["params"] = m.flat_parameters().clone()
    out["buffers"] = m.flat_buffers().clone()
    return out, ran


@pytest.mark.parametrize("grid", [3, 5])
@pytest.mark.parametrize("shape", [(2, 5, 64, 64), (1, 5, 96, 96)], ids=["b2_64x64", "b1_96x96"])
def test_whole_step_fused_equals_separate(dev, states, shape, grid):
    pins = dict(FLAIR_BWD16_WGS=grid, FLAIR_WGH_WGS=grid, FLAIR_HALO_P_WGS=grid)
    with _tuned(FLAIR_BWD16_FUSE=0, **pins):
        sep, ran_sep = _steps(dev, states, 13, shape, "bf16")
    with _tuned(FLAIR_BWD16_FUSE=1, **pins):
        fus, ran_fus = _steps(dev, states, 13, shape, "bf16")
    # the launches: both fused kernels once per step; the apply pass of decoder block 4's second convolution and the two 16-channel
    # weight-gradient launches are gone, and one 16-channel data gradient of the two stays (decoder block 4's first convolution)
    assert not any(k.startswith("bwd16_fused") for k in ran_sep), ran_sep
    assert [ran_fus.get(k, 0) for k in FUSED] == [STEPS, STEPS], ran_fus
    assert ran_fus["bn_bwd_apply"] == ran_sep["bn_bwd_apply"] - STEPS
    assert ran_fus.get("wgrad3x3_halo_bf16_ck16", 0) == ran_sep["wgrad3x3_halo_bf16_ck16"] - 2 * STEPS
    assert ran_fus["bn_bwd_finalize"] == ran_sep["bn_bwd_finalize"]
    for s in range(STEPS):
        assert torch.equal(fus["loss"][s].view(torch.int32), sep["loss"][s].view(torch.int32)), (s, fus["loss"][s].item(), sep["loss"][s].item())
        d = (fus["grads"][s] != sep["grads"][s]).nonzero()
        assert d.numel() == 0, (s, d.numel(), int(d[0]), int(d[-1]), float((fus["grads"][s] - sep["grads"][s]).abs().max()))
        assert bool(torch.isfinite(fus["grads"][s]).all()) and float(fus["grads"][s].abs().max()) > 0
    assert torch.equal(fus["params"], sep["params"])
    assert torch.equal(fus["buffers"], sep["buffers"])


def _assert_same_steps(fus, sep):
    for s in range(STEPS):
        assert torch.equal(fus["loss"][s].view(torch.int32), sep["loss"][s].view(torch.int32)), (s, fus["loss"][s].item(), sep["loss"][s].item())
        d = (fus["grads"][s] != sep["grads"][s]).nonzero()
        assert d.numel() == 0, (s, d.numel(), int(d[0]), int(d[-1]), float((fus["grads"][s] - sep["grads"][s]).abs().max()))
    assert torch.equal(fus["params"], sep["params"])
    assert torch.equal(fus["buffers"], sep["buffers"])


def test_default_grids_above_the_grid_size(dev, states):
    shape = (4, 5, 256, 512)
    with _tuned(FLAIR_BWD16_FUSE=0):
        sep, ran_sep = _steps(dev, states, 13, shape, "bf16")
    with _tuned(FLAIR_BWD16_FUSE=1):
        fus, ran_fus = _steps(dev, states, 13, shape, "bf16")
    assert not any(k.startswith("bwd16_fused") for k in ran_sep), ran_sep
    assert [ran_fus.get(k, 0) for k in FUSED] == [STEPS, STEPS], ran_fus
    _assert_same_steps(fus, sep)


def test_workspace_plan_follows_the_fused_sequence(dev, states):
    from flair_amd import _lib as L
    import flair_amd
    B, H, W = 2, 64, 64
    shape = (B, 5, H, W)
    m = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=13, compute_dtype="bf16").to(dev)
    need = lambda mode: L.lib().flair_unet_workspace_bytes(m._h, B, H, W, mode)
    with _tuned(FLAIR_BWD16_FUSE=0):
        n_sep = need(2)
    with _tuned(FLAIR_BWD16_FUSE=1):
        n_fus, n_bound = need(2), need(1)
        dy = B * H * W * 16 * 2                           # decoder block 4's second convolution: 16 channels of bf16, full resolution
        assert dy % 256 == 0 and n_sep - n_fus == dy, (n_sep, n_fus, dy)
        assert 0 < n_fus < n_bound
        ref, _ = _steps(dev, states, 13, shape, "bf16")

        def exact_workspace(model):
            model._ws_need[(B, H, W, True)] = n_fus
            model._ws["train"] = torch.empty(n_fus, dtype=torch.uint8, device=dev)

        got, ran = _steps(dev, states, 13, shape, "bf16", prepare=exact_workspace)
    assert [ran.get(k, 0) for k in FUSED] == [STEPS, STEPS], ran
    _assert_same_steps(got, ref)


@pytest.mark.parametrize("classes,dtype,head,unit", [(19, "bf16", 0, 1), (13, "f32", 0, 0)], ids=["19_classes", "fp32"])
def test_fallbacks_launch_the_separate_kernels(dev, states, classes, dtype, head, unit):
    with _tuned(FLAIR_BWD16_FUSE=1):
        out, ran = _steps(dev, states, classes, (1, 5, 64, 64), dtype)
    assert [ran.get(k, 0) for k in FUSED] == [head * STEPS, unit * STEPS], ran
    wg = "wgrad3x3_halo_bf16_ck16" if dtype == "bf16" else "wgrad3x3_halo_f32"
    assert ran.get(wg, 0) >= STEPS, ran                      # the head's weight gradient at least
    assert bool(torch.isfinite(out["grads"][-1]).all())


def test_operator_refuses_untileable_shapes(dev):
    from flair_amd import ops
    v = torch.ones(16, device=dev)
    w = torch.zeros(13, 16, 3, 3, device=dev)
    for H, W in ((36, 64), (40, 48)):
        t = torch.zeros(1, H, W, 16, dtype=torch.bfloat16, device=dev)
        assert ops.bwd16_ex(t, t, v, v, w, v, v, rc=True) == -2


# ------------------------------------------------------------------------------------------------ exact arithmetic
def _nhwc(x, dev):
    return x.permute(0, 2, 3, 1).contiguous().to(device=dev, dtype=torch.bfloat16)


def _nchw(y):
    return y.float().cpu().permute(0, 3, 1, 2).double()


def _bf16_exact(t):
    return torch.equal(t.float().to(torch.bfloat16).double(), t.double())


@pytest.fixture(scope="module")
def exact_refs():
    """fp64 references per (flavour, shape): built once, shared by the grids, never modified"""
    built = {}

    def ref(unit, shape):
        key = (unit, shape)
        if key in built:
            return built[key]
        N, H, W = shape
        Cout = 16 if unit else 13
        g = torch.Generator().manual_seed(H + 7 * unit)
        col = lambda v: v.double().view(1, -1, 1, 1)
        r = {}
        r["g"] = E.ternary((N, 16, H, W), g, 0.5)                   # (head: the three padded columns hold values too, nothing may use them)
        r["x"] = E.ints((N, 16, H, W), g, -3, 3)
        r["in_scale"], r["in_shift"] = E.ints((16,), g, -2, 2), E.ints((16,), g, -1, 1)
        r["bsc"], r["bsh"] = E.ints((16,), g, -2, 2), E.ints((16,), g, -1, 1)
        r["w"] = E.ternary((Cout, 16, 3, 3), g, 0.25)
        dy = r["g"].double()
        if unit:
            r["gy"] = E.ints((N, 16, H, W), g, -2, 2)
            r["coef"] = torch.stack([E.ints((16,), g, -2, 2), E.ints((16,), g, -1, 1), E.ints((16,), g, -1, 1)])
            r["gmsc"], r["gmsh"] = E.ints((16,), g, -2, 2), E.ints((16,), g, -1, 1)
            gm = (r["gy"].double() * col(r["gmsc"]) + col(r["gmsh"])) > 0
            assert 0.2 < float(gm.double().mean()) < 0.8
            dy = col(r["coef"][0]) * (dy * gm) + col(r["coef"][1]) * r["gy"].double() + col(r["coef"][2])
        a = torch.relu(r["x"].double() * col(r["in_scale"]) + col(r["in_shift"]))
        wd = r["w"].double()
        r["dx"] = torch.nn.grad.conv2d_input((N, 16, H, W), wd, dy[:, :Cout], padding=1)
        r["dw"] = torch.nn.grad.conv2d_weight(a, wd.shape, dy[:, :Cout], padding=1)
        r["dbias"] = dy[:, :Cout].sum((0, 2, 3))
        m = ((r["x"].double() * col(r["bsc"]) + col(r["bsh"])) > 0).double()
        assert 0.2 < float(m.mean()) < 0.8
        r["s"] = torch.stack([(r["dx"] * m).sum((0, 2, 3)), (r["dx"] * m * r["x"].double()).sum((0, 2, 3))])
        # the exact range: what is stored in bf16 is representable, every fp32 sum stays an integer below 2^24
        assert _bf16_exact(dy) and _bf16_exact(a) and _bf16_exact(r["dx"]), "a stored tensor leaves the exact bf16 range"
        for k in ("dw", "dbias", "s"):
            assert float(r[k].abs().max()) < 2 ** 24
        assert float(r["dx"].abs().max()) > 8 and float(r["dw"].abs().max()) > 8
        built[key] = r
        return r

    return ref


@pytest.mark.parametrize("grid", [1, 3, 0], ids=["grid1", "grid3", "default"])
@pytest.mark.parametrize("shape", [(2, 16, 64), (1, 24, 96)], ids=["b2_16x64", "b1_24x96"])
@pytest.mark.parametrize("unit", [0, 1], ids=["head", "unit"])
def test_fused_kernel_exact(dev, exact_refs, unit, shape, grid):
    from flair_amd import ops
    r = exact_refs(unit, shape)
    f = lambda k: r[k].to(dev)
    kw = {}
    if unit:
        kw = dict(gy=_nhwc(r["gy"], dev), gcoef=r["coef"].contiguous().to(dev), gmsc=f("gmsc"), gmsh=f("gmsh"))
    x = _nhwc(r["x"], dev)
    with _tuned(FLAIR_BWD16_WGS=grid):
        got, ran = _profiled(lambda: ops.bwd16_ex(_nhwc(r["g"], dev), x, f("in_scale"), f("in_shift"), f("w"), f("bsc"), f("bsh"),
                                                  want_dbias=not unit, **kw))
    ntiles = shape[0] * shape[1] * shape[2] // 256
    assert got["rows"] == (min(grid, ntiles) if grid else ntiles), got["rows"]
    assert ran.get(FUSED[unit], 0) == 1 and not any(k.startswith(("conv3x3", "wgrad3x3", "bn_bwd")) for k in ran), ran
    assert torch.equal(_nchw(got["dx"]), r["dx"]), int((_nchw(got["dx"]) != r["dx"]).sum())
    assert not bool(torch.isnan(got["partial"]).any())
    assert torch.equal(got["partial"].double().sum(2).cpu(), r["s"])
    assert torch.equal(got["dw"].double().cpu(), r["dw"]), float((got["dw"].double().cpu() - r["dw"]).abs().max())
    if not unit:
        assert torch.equal(got["dbias"].double().cpu(), r["dbias"])
    assert torch.equal(_nchw(x), r["x"].double())
