"""Case table and references of the exact tests for where the bf16 U-Net kernels round (test_gpu_rounding_exact.py,
test_rounding_cases_cpu.py).

exact_cases.py and bwd_fused_cases.py keep every output within +-256, where a bf16 store never rounds: they pin terms, loops, wraps
and caps and are blind to WHERE a kernel rounds.  The cases here use "integer-beyond-256" data: every input is exactly representable
in bf16, every accumulation is exact in fp32 in any order (sum of magnitudes below 2^24, in units of the common power of two where
values are dyadic fractions), and the results need more than 8 significant bits, so every bf16 store rounds.  The expectation is the
fp64 CPU computation with rf(t) = t.to(bfloat16).double() applied at exactly the points the code documents, the comparison is
torch.equal; in fp32 the same case runs with rf = identity (nothing rounds there).

Every expectation is a function of rf, so the CPU test can evaluate it under round-to-nearest-even (right), under truncation toward
zero (wrong) and with the rounding misplaced (wrong=True: statistics / partial sums of unrounded values, or one rounding at the end
instead of two) and assert that the cases tell them apart.  This module needs no device."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

import bwd_fused_cases as B
import exact_cases as E
from bwd_fused_cases import _gen, _v, dyadic_bits, round_once
from exact_cases import DTYPES, EXACT, ints, ternary


def rne(t):
    """what a bf16 store keeps: round to nearest, ties to even"""
    return round_once(t, "bf16")


def ident(t):
    return t.double()


def trunc(t):
    """the wrong store: bf16 by truncation toward zero (t holds fp32-exact values)"""
    f = t.float()
    assert torch.equal(f.double(), t.double())
    return (f.contiguous().view(torch.int32) & -65536).view(torch.float32).double()


ROUND = {"f32": ident, "bf16": rne}

# |x| sqrt(Cin) ~ 120 with ternary weights at density 0.5: outputs reach +-600, a few per cent of them past +-256, and the largest
# per-channel sum of squares over 256 pixels stays below 2^24 (measured 6.3e6)
XR = {8: 23, 16: 31, 32: 23, 64: 15, 128: 11}
LAZY_SCALES = (1.25, 0.75, -0.625, 1.0, 0.0)
EPI_SCALES = (0.5, 0.75, 1.25, -1.0)


def per_channel(values, Cc, g):
    """[Cc] fp32 drawn from `values`, every one of them present (Cc >= len(values))"""
    sel = (torch.arange(Cc) % len(values))[torch.randperm(Cc, generator=g)]
    return torch.tensor(values, dtype=torch.float32)[sel].contiguous()


# ------------------------------------------------------------------------------------------------ conditions
def store_report(pre):
    """What a bf16 store does to the fp64 values `pre`: fraction changed, how many grow / shrink in magnitude, how many exact ties"""
    pre = pre.double().flatten()
    got, a = rne(pre), pre.abs()
    _, e = torch.frexp(a)                                       # a = m 2^e with m in [0.5, 1): bf16 values are 2^(e - 8) apart
    half = torch.ldexp(torch.ones_like(a), e - 9)
    tie = (a > 0) & (torch.remainder(a, 2 * half) == half)
    return {"changed": float((got != pre).double().mean()), "up": int((got.abs() > a).sum()), "down": int((got.abs() < a).sum()),
            "ties": int(tie.sum())}


def check_store(what, pre, least=0.01):
    """A bf16 store of `pre` rounds: at least 1 % of the elements change, upward, downward and on exact ties, and truncation toward
    zero would give other bits."""
    rep = store_report(pre)
    assert rep["changed"] >= least and rep["up"] and rep["down"] and rep["ties"], (what, rep)
    assert not torch.equal(trunc(pre), rne(pre)), (what, "truncation is not told from rounding")
    return rep


def check_bf16_inputs(what, tensors):
    for k, t in tensors.items():
        if t is not None and t.dtype == torch.float32:
            assert torch.equal(t.to(torch.bfloat16).float(), t), (what, k, "is not a bf16 value")


def check_sum(what, magnitudes, like=None):
    """sum of |terms| below 2^24 in the unit of the smallest fraction the terms have (`like`: a tensor that holds those fractions)"""
    q = dyadic_bits(like)[0] if like is not None else 0
    top = float(magnitudes.double().abs().max()) * 2.0 ** q
    assert top < EXACT, (what, "sum of magnitudes", top, "in units of 2^-%d" % q)
    return top


def differs(a, b):
    """fraction of elements in which two expectations differ"""
    return float((a.double() != b.double()).double().mean())


# ------------------------------------------------------------------------------------------------ a - d. convolution forms
@dataclass(frozen=True)
class RCase:
    name: str
    form: str          # fwd | epilogue | accumulate | acc_src | pool | lazy
    N: int
    H: int
    W: int
    C0: int
    Cout: int
    R: int = 3
    stride: int = 1
    pad: int = 1
    xr: int = 0                  # |x| <= xr (default XR[C0])
    stats: bool = True           # fwd only
    bias: bool = False
    nchw: bool = False
    real_cin: int = 0
    pool_c0: int = 0
    accumulate: bool = False     # pool: the pooled half adds into a pre-filled gradient
    skip_accumulate: bool = False
    kernel: object = field(default=None, compare=False)

    @property
    def mode(self):
        return 1 if self.form in ("accumulate", "acc_src", "pool") else 0

    @property
    def Ho(self):
        return (self.H + 2 * self.pad - self.R) // self.stride + 1

    @property
    def Wo(self):
        return (self.W + 2 * self.pad - self.R) // self.stride + 1

    def want(self, dt):
        return self.kernel[dt] if isinstance(self.kernel, dict) else self.kernel

    def launch(self, dt):
        """(family, profile name) by the restated dispatch of exact_cases"""
        if self.form == "fwd":
            has_out = self.Cout % 8 == 0
            return E.conv_kernel(dt, self.N, self.H, self.W, self.Ho, self.Wo, self.C0, 0, self.Cout, self.R, self.stride, 1, self.pad,
                                 has_out=has_out, nchw=self.nchw or not has_out, stats=self.stats, bias=self.bias)
        return E.conv_kernel(dt, self.N, self.H, self.W, self.H, self.W, self.C0, 0, self.Cout, 3, 1, 1, 1, in_scale=self.form == "lazy",
                             pool_c0=self.pool_c0, epilogue=self.form == "epilogue", bias=self.form == "epilogue")


_HG128 = {"f32": "hg_n128", "bf16": "halo"}
CONV_CASES = [
    # a. forward: out = rf(acc [+ bias]), s1 = sum out, s2 = sum out^2 (conv_hg.hip / conv_halo.hip / conv_igemm.hip / stem.hip
    #    "statistics of the ROUNDED outputs"; tile_direct.h direct_store "s1 / s2: ... of the ROUNDED outputs")
    RCase("fwd_hg64to64", "fwd", 1, 8, 32, 64, 64, kernel="hg_n64"),
    RCase("fwd_hg64to128", "fwd", 1, 8, 16, 64, 128, kernel="hg_n128"),
    RCase("fwd_hg64to32", "fwd", 1, 8, 32, 64, 32, kernel="hg_n32"),
    RCase("fwd_p16to16", "fwd", 1, 8, 32, 16, 16, kernel="halo_p"),
    RCase("fwd_p32to32", "fwd", 1, 8, 32, 32, 32, kernel={"f32": "hg_n32", "bf16": "halo_p"}),
    RCase("fwd_t32to128_stats", "fwd", 1, 8, 32, 32, 128, kernel=_HG128),
    RCase("fwd_pm32to128", "fwd", 1, 8, 32, 32, 128, stats=False, kernel={"f32": "hg_n128", "bf16": "halo_pm"}),
    RCase("fwd_g3x3s2_64to128", "fwd", 1, 16, 32, 64, 128, stride=2, kernel="igemm"),
    RCase("fwd_stem", "fwd", 1, 16, 32, 8, 64, R=7, stride=2, pad=3, real_cin=5, kernel={"f32": "igemm", "bf16": "stem"}),
    # the head: 13 logits + integer bias, the fp32 NCHW copy holds the ROUNDED values (direct_store writes v[][], the gather-form
    # kernel reads its C tile back)
    RCase("fwd_head_p16to13", "fwd", 1, 8, 32, 16, 13, bias=True, nchw=True, stats=False, kernel="halo_p"),
    RCase("fwd_head_g16to13", "fwd", 1, 12, 20, 16, 13, bias=True, nchw=True, stats=False, kernel="igemm"),
    # b. inference epilogue: rf([relu](rf(acc oscale + oshift + bias) + ores)) (store_tile / direct_store / the gather-form
    #    kernel's store loop: the C tile, or v[][], is rounded before the residual is added)
    RCase("epi_hg64to64", "epilogue", 1, 8, 32, 64, 64, kernel="hg_n64"),
    RCase("epi_p16to16", "epilogue", 1, 8, 32, 16, 16, kernel="halo_p"),
    RCase("epi_p32to32", "epilogue", 1, 8, 32, 32, 32, kernel={"f32": "hg_n32", "bf16": "halo_p"}),
    RCase("epi_g64to64", "epilogue", 1, 10, 12, 64, 64, kernel="igemm_bm32"),
    # c. data gradient (mode 1).  accumulate / acc_src: rf(rf(acc) + prev) ("store_tile rounds before it accumulates")
    RCase("acc_hg64to64", "accumulate", 1, 8, 32, 64, 64, kernel="hg_n64"),
    RCase("acc_hg64to128", "accumulate", 1, 8, 16, 64, 128, kernel="hg_n128"),
    RCase("acc_p16to16", "accumulate", 1, 8, 32, 16, 16, kernel="halo_p"),
    RCase("acc_p32to32", "accumulate", 1, 8, 32, 32, 32, kernel={"f32": "hg_n32", "bf16": "halo_p"}),
    RCase("accsrc_hg64to64", "acc_src", 1, 8, 32, 64, 64, kernel="hg_n64"),
    RCase("accsrc_hg64to128", "acc_src", 1, 8, 16, 64, 128, kernel="hg_n128"),
    #    pool_c0: pooled columns rf(((rf(a0) + rf(a1)) + rf(a2)) + rf(a3) [+ prev]), skip columns rf(acc) or rf(rf(acc) + prev_skip)
    RCase("pool_hg64to192_c64_skipacc", "pool", 1, 8, 32, 64, 192, pool_c0=64, skip_accumulate=True, kernel="hg_n64"),
    RCase("pool_hg64to192_c128_acc", "pool", 1, 8, 32, 64, 192, pool_c0=128, accumulate=True, kernel="hg_n64"),
    RCase("pool_hg64to128_all", "pool", 1, 8, 16, 64, 128, pool_c0=128, kernel="hg_n128"),
    RCase("pool_hg64to256_c128_acc_skipacc", "pool", 1, 8, 16, 64, 256, pool_c0=128, accumulate=True, skip_accumulate=True, kernel="hg_n128"),
    RCase("pool_p16to16_all", "pool", 1, 8, 32, 16, 16, pool_c0=16, kernel="halo_p"),
    RCase("pool_p16to32_all_acc", "pool", 1, 8, 32, 16, 32, pool_c0=32, accumulate=True, kernel="halo_p"),
    RCase("pool_t32to96_c32_skipacc", "pool", 1, 8, 32, 32, 96, pool_c0=32, skip_accumulate=True, kernel="halo"),
    # d. lazy BatchNorm + ReLU input: x' = rf(relu(fmaf(x, s, sh))) (chunk_bn_relu: "the bn_act arithmetic"), then the exact
    #    convolution of x'
    RCase("lazy_hg64to64", "lazy", 1, 8, 32, 64, 64, xr=255, kernel="hg_n64"),
    RCase("lazy_p16to16", "lazy", 1, 8, 32, 16, 16, xr=255, kernel="halo_p"),
    RCase("lazy_p32to32", "lazy", 1, 8, 32, 32, 32, xr=255, kernel="halo_p"),
    RCase("lazy_pm32to128", "lazy", 1, 8, 32, 32, 128, xr=255, kernel={"f32": "hg_n128", "bf16": "halo_pm"}),
]


def _sum4(p):
    """2x2 sum pool in store_tile's order: ((y, x) + (y, x+1)) + (y+1, x)) + (y+1, x+1)"""
    return ((p[:, :, 0::2, 0::2] + p[:, :, 0::2, 1::2]) + p[:, :, 1::2, 0::2]) + p[:, :, 1::2, 1::2]


@functools.lru_cache(maxsize=4)
def conv_reference(c):
    """Seeded inputs (fp32 CPU, NCHW / OIHW; mode 1: w is the forward layer's [C0][Cout][3][3]) and the exact accumulator (fp64)."""
    g = _gen(c.name)
    xr = c.xr or XR[c.C0]
    x = ints((c.N, c.C0, c.H, c.W), g, -xr, xr)
    w = ternary((c.C0, c.Cout, 3, 3) if c.mode else (c.Cout, c.C0, c.R, c.R), g, 0.5)
    if c.real_cin:
        x[:, c.real_cin:] = 0
        w[:, c.real_cin:] = 0
    r = {"x": x, "w": w}
    wd = w.double()
    conv = (lambda t: F.conv_transpose2d(t, wd, padding=1)) if c.mode else (lambda t: F.conv2d(t, wd, stride=c.stride, padding=c.pad))
    r["conv"] = conv
    xin = x.double()
    if c.form == "lazy":
        r["in_scale"], r["in_shift"] = per_channel(LAZY_SCALES, c.C0, g), ints((c.C0,), g, -5, 5) / 2
        xin = torch.relu(xin * _v(r["in_scale"]) + _v(r["in_shift"]))     # exact: quarters and eighths of integers below 2^9
        r["xpre"] = xin
    r["acc"] = conv(xin)
    wabs = wd.abs()
    r["acc_abs"] = (F.conv_transpose2d(xin.abs(), wabs, padding=1) if c.mode else F.conv2d(xin.abs(), wabs, stride=c.stride, padding=c.pad))
    oshape = tuple(r["acc"].shape)
    if c.bias:
        r["bias"] = ints((c.Cout,), g, -3, 3)
    if c.form == "epilogue":
        r["oscale"], r["oshift"], r["bias"] = per_channel(EPI_SCALES, c.Cout, g), ints((c.Cout,), g, -3, 3), ints((c.Cout,), g, -3, 3)
        r["ores"] = ints(oshape, g, -200, 200)
    if c.form in ("accumulate", "acc_src"):
        r["prev"] = ints(oshape, g, -255, 255)
    if c.form == "pool":
        r["prev"] = ints((c.N, c.pool_c0, c.H // 2, c.W // 2), g, -255, 255) if c.accumulate else None
        r["prev_skip"] = ints((c.N, c.Cout - c.pool_c0, c.H, c.W), g, -255, 255) if c.skip_accumulate else None
    return r


def conv_expect(c, r, rf, wrong=False):
    """The expectation of one case under the store rounding rf.  wrong: the rounding misplaced (see the module docstring)."""
    acc = r["acc"]
    o = {}
    if c.form == "fwd":
        pre = acc + (_v(r["bias"]) if c.bias else 0)
        o["y"] = rf(pre)
        src = pre if wrong else o["y"]
        if c.stats:
            o["s1"], o["s2"] = src.sum(dim=(0, 2, 3)), (src * src).sum(dim=(0, 2, 3))
    elif c.form == "epilogue":
        pre = acc * _v(r["oscale"]) + (_v(r["oshift"]) + _v(r["bias"]))
        staged = pre if wrong else rf(pre)
        o["y_relu"] = rf(torch.relu(staged + r["ores"].double()))
        o["y_lin"] = rf(staged + r["ores"].double())
    elif c.form in ("accumulate", "acc_src"):
        o["y"] = rf((acc if wrong else rf(acc)) + r["prev"].double())
    elif c.form == "pool":
        a = acc if wrong else rf(acc)
        s4 = _sum4(a[:, :c.pool_c0])
        o["y"] = rf(s4 + (r["prev"].double() if c.accumulate else 0))
        if c.pool_c0 < c.Cout:
            o["skip"] = rf(a[:, c.pool_c0:] + r["prev_skip"].double()) if c.skip_accumulate else rf(acc[:, c.pool_c0:])
    elif c.form == "lazy":
        o["xp"] = r["xpre"] if wrong else rf(r["xpre"])
        o["y"] = rf(r["conv"](o["xp"]))
    return o


def check_conv_case(c):
    """Every condition of one convolution case, on the reference alone.  Returns the measured figures."""
    r = conv_reference(c)
    check_bf16_inputs(c.name, {k: v for k, v in r.items() if isinstance(v, torch.Tensor)})
    for dt in DTYPES:
        assert c.launch(dt)[0] == c.want(dt), (c.name, dt, c.launch(dt))
    fig = {"acc": check_sum(c.name + " acc", r["acc_abs"], r.get("xpre"))}
    good, bad, cut = (conv_expect(c, r, f, w) for f, w in ((rne, False), (rne, True), (trunc, False)))
    exact = conv_expect(c, r, ident)
    if c.form == "fwd":
        fig["y"] = check_store(c.name + " y", exact["y"])
        if c.stats:
            check_sum(c.name + " s1", good["y"].abs().sum(dim=(0, 2, 3)))
            fig["s2"] = check_sum(c.name + " s2", good["s2"])
            assert differs(good["s1"], bad["s1"]) >= 0.5 and differs(good["s2"], bad["s2"]) >= 0.5, (c.name, "statistics of unrounded outputs")
            assert not torch.equal(good["s1"], cut["s1"]) and not torch.equal(good["s2"], cut["s2"])
    elif c.form == "epilogue":
        pre = r["acc"] * _v(r["oscale"]) + (_v(r["oshift"]) + _v(r["bias"]))
        assert dyadic_bits(pre)[1] < EXACT
        check_store(c.name + " staged", pre)
        check_store(c.name + " y_lin", rne(pre) + r["ores"].double())
        check_store(c.name + " y_relu", torch.relu(rne(pre) + r["ores"].double()))
        fig["two roundings"] = (differs(good["y_lin"], bad["y_lin"]), differs(good["y_relu"], bad["y_relu"]))
        assert min(fig["two roundings"]) >= 0.005, (c.name, fig)
    elif c.form in ("accumulate", "acc_src"):
        check_store(c.name + " acc", r["acc"])
        check_store(c.name + " y", rne(r["acc"]) + r["prev"].double())
        fig["two roundings"] = differs(good["y"], bad["y"])
        assert fig["two roundings"] >= 0.005, (c.name, fig)
    elif c.form == "pool":
        check_store(c.name + " acc", r["acc"])
        a = rne(r["acc"])
        s4abs = _sum4(a[:, :c.pool_c0].abs()) + (r["prev"].double().abs() if c.accumulate else 0)
        check_sum(c.name + " pool", s4abs)
        check_store(c.name + " y", _sum4(a[:, :c.pool_c0]) + (r["prev"].double() if c.accumulate else 0))
        fig["two roundings"] = differs(good["y"], bad["y"])
        assert fig["two roundings"] >= 0.02, (c.name, fig)
        if c.skip_accumulate:
            assert differs(good["skip"], bad["skip"]) >= 0.005, c.name
    elif c.form == "lazy":
        fig["xp"] = check_store(c.name + " x'", r["xpre"])
        check_store(c.name + " y", r["conv"](rne(r["xpre"])))
        assert differs(good["y"], bad["y"]) > 0, (c.name, "one rounding at the end")
        assert not torch.equal(good["xp"], cut["xp"])
    for k in good:
        if k not in ("s1", "s2"):
            assert not torch.equal(good[k], cut[k]), (c.name, k, "truncation is not told from rounding")
    return fig


# ------------------------------------------------------------------------------------------------ c. fused BatchNorm-backward sums
BNR_CASES = [
    # sums of the STORED gradient d: sum d m, sum d m y (store_tile bnr_item "v: the stored (rounded) gradient chunk";
    # DirectBnr::item "rounded here as store_tile's bnr_item sees them"); mask from y / from `out`; masked store; pooled half
    B.BnrCase("rbnr_hg64to64", 1, 8, 32, 64, 64, kernel="hg_n64"),
    B.BnrCase("rbnr_out_acc_hg64to64", 1, 8, 32, 64, 64, from_out=True, accumulate=True, kernel="hg_n64"),
    B.BnrCase("rbnr_mask_accsrc_hg64to128", 1, 8, 16, 64, 128, bnr_mask=True, accumulate=True, acc_src=True, kernel="hg_n128"),
    B.BnrCase("rbnr_out_mask_hg64to128", 1, 8, 16, 64, 128, from_out=True, bnr_mask=True, kernel="hg_n128"),
    B.BnrCase("rbnr_pool_hg64to128_all", 1, 8, 16, 64, 128, pool_c0=128, kernel="hg_n128"),
    B.BnrCase("rbnr_pool_mask_hg64to192_c64_skipacc", 1, 8, 32, 64, 192, pool_c0=64, bnr_mask=True, skip_accumulate=True, kernel="hg_n64"),
    B.BnrCase("rbnr_p16to16", 1, 8, 32, 16, 16, kernel="halo_p"),
    B.BnrCase("rbnr_acc_p32to32", 1, 8, 32, 32, 32, accumulate=True, kernel="halo_p"),
    B.BnrCase("rbnr_pool_p16to16_all", 1, 8, 32, 16, 16, pool_c0=16, kernel="halo_p"),
]


@functools.lru_cache(maxsize=4)
def bnr_reference(c):
    g = _gen(c.name)
    xr = XR[c.C0]
    r = {"x": ints((c.N, c.C0, c.H, c.W), g, -xr, xr), "w": ternary((c.C0, c.Cout, 3, 3), g, 0.5)}
    r["acc"] = F.conv_transpose2d(r["x"].double(), r["w"].double(), padding=1)
    r["acc_abs"] = F.conv_transpose2d(r["x"].double().abs(), r["w"].double().abs(), padding=1)
    dshape = (c.N, c.pool_c0, c.H // 2, c.W // 2) if c.pool_c0 else tuple(r["acc"].shape)
    r["prev"] = ints(dshape, g, -255, 255) if c.accumulate else None
    r["prev_skip"] = ints((c.N, c.Cout - c.pool_c0, c.H, c.W), g, -255, 255) if c.skip_accumulate else None
    r["y"], r["scale"], r["shift"], r["out"], r["m"] = B.mask_inputs(g, dshape, c.from_out)
    return r


def bnr_expect(c, r, rf, wrong=False):
    """stored: what the launch leaves in `out`; s1 / s2: the sums of its partial.  wrong: the sums of the unrounded gradient."""
    acc = r["acc"]
    prev = r["prev"].double() if c.accumulate else 0
    o = {}
    if c.pool_c0:
        d = rf(_sum4(rf(acc)[:, :c.pool_c0]) + prev)
        exact = _sum4(acc[:, :c.pool_c0]) + prev
        if c.pool_c0 < c.Cout:
            o["skip"] = rf(rf(acc[:, c.pool_c0:]) + r["prev_skip"].double()) if c.skip_accumulate else rf(acc[:, c.pool_c0:])
    else:
        d = rf(rf(acc) + prev)
        exact = acc + prev
    m, y = r["m"], r["y"].double()
    o["stored"] = d * m if c.bnr_mask else d
    src = exact if wrong else d
    o["s1"], o["s2"] = (src * m).sum(dim=(0, 2, 3)), (src * m * y).sum(dim=(0, 2, 3))
    o["sabs"] = (src * m * y).abs().sum(dim=(0, 2, 3))
    return o


def check_bnr_case(c):
    r = bnr_reference(c)
    check_bf16_inputs(c.name, {k: r[k] for k in ("x", "w", "prev", "prev_skip", "y", "out", "scale", "shift")})
    B.check_bnr_dispatch_and_loops(c)
    B.check_mask_variety(c.name, r["y"], r["scale"], r["shift"])
    check_sum(c.name + " acc", r["acc_abs"])
    good, bad, cut = bnr_expect(c, r, rne), bnr_expect(c, r, rne, True), bnr_expect(c, r, trunc)
    check_store(c.name + " acc", r["acc"])
    a = rne(r["acc"])
    if c.pool_c0 or c.accumulate:      # the final store of the gradient: rf(rf(acc) + prev) or rf(sum of four rf(acc) [+ prev])
        check_store(c.name + " d", (_sum4(a[:, :c.pool_c0]) if c.pool_c0 else a) + (r["prev"].double() if c.accumulate else 0))
    if c.skip_accumulate:
        check_store(c.name + " skip", a[:, c.pool_c0:] + r["prev_skip"].double())
    check_sum(c.name + " sum |d m|", (good["stored"] * r["m"]).abs().sum(dim=(0, 2, 3)))
    check_sum(c.name + " sum |d m y|", good["sabs"])
    if c.pool_c0:
        check_sum(c.name + " pool", _sum4(rne(r["acc"])[:, :c.pool_c0].abs()) + (r["prev"].double().abs() if c.accumulate else 0))
    fig = {"s1": differs(good["s1"], bad["s1"]), "s2": differs(good["s2"], bad["s2"])}
    assert fig["s1"] >= 0.5 and fig["s2"] >= 0.5, (c.name, "sums of the unrounded gradient", fig)
    for k in ("stored", "s1", "s2"):
        assert not torch.equal(good[k], cut[k]), (c.name, k, "truncation is not told from rounding")
    if c.from_out:
        my = (r["y"].double() * _v(r["scale"]) + _v(r["shift"]) > 0).double()
        assert float((my != r["m"]).double().mean()) > 0.2
    return fig


# ------------------------------------------------------------------------------------------------ c. parity-class stride-2 gradient
PARITY_CASE = B.ParityCase("rpar_64to128_accumulate", 1, 5, 7, 64, 128, accumulate=True)
PARITY_XR = 31


@functools.lru_cache(maxsize=1)
def parity_reference():
    c = PARITY_CASE
    g = _gen(c.name)
    dy = ints((c.N, c.Cf_out, c.Ho, c.Wo), g, -PARITY_XR, PARITY_XR)
    w = ternary((c.Cf_out, c.Cf_in, 3, 3), g, 0.5)
    xshape = (c.N, c.Cf_in, 2 * c.Ho, 2 * c.Wo)
    acc = torch.nn.grad.conv2d_input(xshape, w.double(), dy.double(), stride=2, padding=1)
    acc_abs = torch.nn.grad.conv2d_input(xshape, w.double().abs(), dy.double().abs(), stride=2, padding=1)
    return {"dy": dy, "w": w, "prev": ints(xshape, g, -255, 255), "acc": acc, "acc_abs": acc_abs}


def parity_expect(r, rf, wrong=False):
    return rf((r["acc"] if wrong else rf(r["acc"])) + r["prev"].double())     # the gather-form store loop: v = C tile (T), then += dst


def check_parity_case():
    c, r = PARITY_CASE, parity_reference()
    check_bf16_inputs(c.name, {k: r[k] for k in ("dy", "w", "prev")})
    for dt in DTYPES:
        assert c.launch(dt)[0] == "igemm"
    check_sum(c.name, r["acc_abs"])
    check_store(c.name + " acc", r["acc"])
    check_store(c.name + " dx", rne(r["acc"]) + r["prev"].double())
    fig = differs(parity_expect(r, rne), parity_expect(r, rne, True))
    assert fig >= 0.005, (c.name, fig)
    assert not torch.equal(parity_expect(r, rne), parity_expect(r, trunc))
    return fig


# ------------------------------------------------------------------------------------------------ d. lazy input of the weight gradient
WLAZY_CASES = [
    E.FusedCase("rwlazy_p16to16", "wgrad_lazy", 1, 8, 32, 16, 16, kernel="halo"),
    E.FusedCase("rwlazy_big64to128", "wgrad_lazy", 1, 8, 16, 64, 128, kernel="big_kg1"),
    E.FusedCase("rwlazy_big64to64", "wgrad_lazy", 1, 8, 32, 64, 64, kernel={"f32": "big_kg1", "bf16": "big_kg2"}),
]


@functools.lru_cache(maxsize=2)
def wlazy_reference(c):
    g = _gen(c.name)
    r = {"x": ints((c.N, c.C0, c.H, c.W), g, -255, 255), "dy": ternary((c.N, c.Cout, c.H, c.W), g, 0.5),
         "in_scale": per_channel(LAZY_SCALES, c.C0, g), "in_shift": ints((c.C0,), g, -5, 5) / 2}
    r["xpre"] = torch.relu(r["x"].double() * _v(r["in_scale"]) + _v(r["in_shift"]))
    return r


def wlazy_expect(c, r, rf, wrong=False):
    xp = r["xpre"] if wrong else rf(r["xpre"])
    return torch.nn.grad.conv2d_weight(xp, (c.Cout, c.C0, 3, 3), r["dy"].double(), padding=1)


def check_wlazy_case(c):
    r = wlazy_reference(c)
    check_bf16_inputs(c.name, {k: r[k] for k in ("x", "dy", "in_scale", "in_shift")})
    for dt in DTYPES:
        assert E.fused_kernel(c, dt)[0] == c.want(dt), (c.name, dt, E.fused_kernel(c, dt)[:2])
    check_store(c.name + " x'", r["xpre"])
    terms = torch.nn.grad.conv2d_weight(r["xpre"].abs(), (c.Cout, c.C0, 3, 3), r["dy"].double().abs(), padding=1)
    check_sum(c.name + " dw", terms, r["xpre"])
    good = wlazy_expect(c, r, rne)
    fig = differs(good, wlazy_expect(c, r, rne, True))
    assert fig > 0 and not torch.equal(good, wlazy_expect(c, r, trunc)), (c.name, fig)
    return fig


# ------------------------------------------------------------------------------------------------ e. stem weight gradient, fused apply
STEM_SHAPE = (1, 16, 32)            # N and the OUTPUT extent: four 8x16 tiles
STEM_K1 = (1.125, 0.875, 1.375, -1.25, 0.625)


@functools.lru_cache(maxsize=1)
def stem_reference():
    """staged = rf(k1 dout m + k2 y + k3) (stem.hip store_tile: fmaf(k1, dm, fmaf(k2, y, k3)), one f_to_chunk into the LDS tile the
    matrix cores read), dw = the exact weight gradient against staged.  Coefficients in eighths."""
    N, Ho, Wo = STEM_SHAPE
    g = _gen("rstem")
    x = ints((N, 8, 2 * Ho, 2 * Wo), g, -XR[8], XR[8])
    x[:, 5:] = 0
    dout = ints((N, 64, Ho, Wo), g, -31, 31)
    y, scale, shift, _, m = B.mask_inputs(g, (N, 64, Ho, Wo), False)
    k1, k2, k3 = per_channel(STEM_K1, 64, g), ints((64,), g, -4, 4) / 8, ints((64,), g, -8, 8) / 8
    pre = _v(k1) * dout.double() * m + _v(k2) * y.double() + _v(k3)
    return {"x": x, "dout": dout, "y": y, "scale": scale, "shift": shift, "coef": torch.stack([k1, k2, k3]), "pre": pre}


def stem_expect(r, rf, wrong=False):
    staged = r["pre"] if wrong else rf(r["pre"])
    return torch.nn.grad.conv2d_weight(r["x"][:, :5].double(), (64, 5, 7, 7), staged, stride=2, padding=3)


def check_stem_case():
    r = stem_reference()
    check_bf16_inputs("rstem", {k: r[k] for k in ("x", "dout", "y", "scale", "shift", "coef")})
    B.check_stem_dispatch(STEM_SHAPE)
    B.check_mask_variety("rstem", r["y"], r["scale"], r["shift"])
    fig = check_store("rstem staged", r["pre"])
    terms = torch.nn.grad.conv2d_weight(r["x"][:, :5].double().abs(), (64, 5, 7, 7), rne(r["pre"]).abs(), stride=2, padding=3)
    check_sum("rstem dw", terms, r["pre"])
    good = stem_expect(r, rne)
    assert differs(good, stem_expect(r, rne, True)) > 0 and not torch.equal(good, stem_expect(r, trunc))
    return fig


# ------------------------------------------------------------------------------------------------ f. elementwise
EW_SHAPE = (2, 8, 12, 64)            # N, H, W, C of the elementwise tensors
BN_EVAL_TARGETS = (1.0, 4.0, 0.25)   # running_var + eps rounds to one of these in fp32: sqrtf gives 1, 2, 0.5 exactly


def running_var_for(target, eps=1e-5):
    """fp32 v with fl(v + eps) == target exactly (bn_eval_coeffs_kernel: gamma / sqrtf(rv + eps))"""
    e = torch.tensor(eps, dtype=torch.float32)
    v = torch.tensor(target, dtype=torch.float32) - e
    for _ in range(8):
        s = v + e
        if float(s) == target:
            return float(v)
        v = torch.nextafter(v, torch.tensor(float("inf") if float(s) < target else float("-inf")))
    raise AssertionError("no fp32 running_var gives %r" % target)


@functools.lru_cache(maxsize=1)
def elementwise_reference():
    N, H, W, Cc = EW_SHAPE
    g = _gen("relementwise")
    shape = (N, Cc, H, W)
    r = {"y": ints(shape, g, -255, 255), "scale": per_channel(LAZY_SCALES, Cc, g), "shift": ints((Cc,), g, -5, 5) / 2}
    r["pre"] = r["y"].double() * _v(r["scale"]) + _v(r["shift"])                    # bn_act: fmaf, [fmaxf], one f_to_chunk
    # bn_act_maxpool: large neighbours, so that rounding makes ties in windows whose unrounded values have a single maximum
    r["ymp"] = ints(shape, g, 224, 255)
    r["pre_mp"] = r["ymp"].double() * _v(r["scale"]) + _v(r["shift"])
    # bn_relu_forward, eval mode, with a residual: rf(relu(fmaf(y, sc, sh) + res)), sc = gamma / sqrt(rv + eps), sh = beta - rm sc
    root = torch.tensor([t ** 0.5 for t in BN_EVAL_TARGETS])[torch.arange(Cc) % 3]
    r["rv"] = torch.tensor([running_var_for(t) for t in BN_EVAL_TARGETS], dtype=torch.float32)[torch.arange(Cc) % 3].contiguous()
    r["gamma"], r["beta"], r["rm"] = per_channel(LAZY_SCALES, Cc, g), ints((Cc,), g, -5, 5) / 2, ints((Cc,), g, -4, 4).float()
    sc = r["gamma"].double() / root.double()
    r["res"] = ints(shape, g, -255, 255)
    r["pre_res"] = r["y"].double() * _v(sc) + _v(r["beta"].double() - r["rm"].double() * sc) + r["res"].double()
    # plain sums of two or five bf16 integers
    r["a"], r["b"] = ints(shape, g, -255, 255), ints(shape, g, -255, 255)
    # max pool backward: gradient of the 3x3 / stride-2 pool of a tensor with ties in every window
    xp = torch.relu(ternary(shape, g, 0.5)).double().requires_grad_(True)
    p = F.max_pool2d(xp, 3, 2, 1)
    r["pool_dy"] = ints(tuple(p.shape), g, -255, 255)
    p.backward(r["pool_dy"].double())
    r["pool_x"], r["pool_dx"] = xp.detach().float(), xp.grad
    # BatchNorm backward with the residual gradient accumulated: dres = rf(prev + dout m)
    r["bn_y"], r["bn_scale"], r["bn_shift"], r["bn_out"], r["bn_m"] = B.mask_inputs(g, shape, True)
    r["bn_mean"], r["bn_invstd"], r["bn_gamma"] = B.bn_params(g, Cc)
    return r


def rounding_ties(pre):
    """3x3 / stride-2 windows of relu(pre) in which the ROUNDED values tie for the maximum and the unrounded ones do not"""
    win = lambda t: F.pad(t, (1, 1, 1, 1), value=float("-inf")).unfold(2, 3, 2).unfold(3, 3, 2).reshape(*t.shape[:2], t.shape[2] // 2, t.shape[3] // 2, 9)
    a, b = win(torch.relu(pre)), win(rne(torch.relu(pre)))
    count = lambda t: (t == t.amax(4, keepdim=True)).sum(4)
    return int(((count(b) > 1) & (count(a) == 1)).sum()), win


def check_elementwise():
    r = elementwise_reference()
    # (rv is an fp32 parameter on both paths: it only has to give an exact fp32 square root, asserted below)
    check_bf16_inputs("elementwise", {k: v for k, v in r.items() if isinstance(v, torch.Tensor) and k != "rv"})
    fig = {"bn_act": check_store("bn_act", r["pre"]), "bn_act relu": check_store("bn_act relu", torch.relu(r["pre"])),
           "residual": check_store("bn_relu_forward + residual", torch.relu(r["pre_res"])),
           "a + b": check_store("a + b", r["a"].double() + r["b"].double())}
    for t in BN_EVAL_TARGETS:
        v = torch.tensor(running_var_for(t), dtype=torch.float32)
        assert float(v + torch.tensor(1e-5, dtype=torch.float32)) == t
    assert dyadic_bits(r["pre_res"])[1] < EXACT
    fig["windows tied by rounding"] = rounding_ties(r["pre_mp"])[0]
    assert fig["windows tied by rounding"] >= 100
    check_store("bn_act_maxpool", torch.relu(r["pre_mp"]))
    fig["pool"] = check_store("max pool backward accumulate", r["pool_dx"] + r["a"].double())
    fig["dres"] = check_store("dres accumulate", r["a"].double() + r["b"].double() * r["bn_m"])
    s4 = _sum4(r["a"].double())
    fig["upcat"] = check_store("upcat_bwd dx0", s4)
    check_store("upcat_bwd dx0 accumulate", s4 + r["b"].double()[:, :, ::2, ::2])
    return fig
