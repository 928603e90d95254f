"""Case table and references of the exact-arithmetic operator tests (test_gpu_ops_exact.py, test_ops_exact_cases_cpu.py).

Activations, weights and incoming gradients are drawn from {-1, 0, 1}.  Every product and every partial sum is then an
integer; while the sum of the magnitudes of the terms stays below 2^24 the result is exact in fp32 in ANY summation order,
and an output within +-256 is exactly representable in bf16.  So the expected result is the fp64 CPU convolution and the
comparison is torch.equal.  The conditions are asserted on the reference alone (check_exact_range), never assumed.

The table is written against the dispatch predicates of csrc (launch_conv, launch_hg_t, conv_halo_applicable,
halo_persistent(_multi), conv_stem_applicable, wg_halo_geom, wg_big_geom, launch_t): the functions conv_kernel / wgrad_kernel
below restate them in plain integer arithmetic, every case names the kernel family it is meant for, the CPU test checks that
the restated dispatch agrees with that intent and the GPU test checks the profile name of what actually ran.
This module needs no device."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

EXACT = float(2 ** 24)
DTYPES = ("f32", "bf16")

# tuning switches the cases touch, with the defaults they are put back to
TUNE_DEFAULTS = {"FLAIR_HALO_P_WGS": 0, "FLAIR_WGH_WGS": 0, "FLAIR_WG_CUS_OP": 256, "FLAIR_IGEMM_BM32": 2}


def ternary(shape, gen, density):
    """{-1, 0, 1} with P(non-zero) = density, fp32."""
    nz = torch.rand(shape, generator=gen) < density
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (nz * sign).to(torch.float32)


def ints(shape, gen, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32)


# ------------------------------------------------------------------------------------------------ dispatch, restated
def _cdiv(a, b):
    return (a + b - 1) // b


def _rup(a, b):
    return _cdiv(a, b) * b


def _pick_bn(cout):
    return 128 if cout >= 128 else 64 if cout >= 64 else 32 if cout >= 32 else 16


def halo_applicable(C0, C1, Cout, R, out_mul, in_div, pad, Hin, Win, Hout, Wout):
    Cin = C0 + C1
    if R != 3 or out_mul != 1 or in_div != 1 or pad != 1:
        return False
    if Hout != Hin or Wout != Win or Hout % 8 or Wout % 32:
        return False
    if Cin == 16:
        return C1 == 0 and Cout <= 32
    if Cin % 32 or C0 % 32:
        return False
    return Cin <= 128 and Cout <= 128 and (Cout <= 32 or Cin <= 32)


def hg_tile_pixels(Hout, Wout, Cout):
    can128 = Wout % 16 == 0 and Hout % 8 == 0
    can256 = (Wout % 32 == 0 and Hout % 8 == 0) or (Wout % 16 == 0 and Hout % 16 == 0)
    if Cout % 128:
        return 256 if can256 else 128 if can128 else 0
    return 128 if can128 else 256 if can256 else 0


def hg_applicable(dt, C0, C1, Cout, R, out_mul, in_div, pad, Hin, Win, Hout, Wout, has_out, nchw, in_scale=False, pool_c0=0, bnr=False):
    """conv_hg_applicable; bnr: ConvArgs::bnr_partial is set."""
    ck = 32 if dt == "f32" else 64
    Cin = C0 + C1
    if R != 3 or out_mul != 1 or in_div != 1 or pad != 1:
        return False
    if Hout != Hin or Wout != Win or nchw or not has_out:
        return False
    if in_scale and bnr:
        return False
    if Cin % ck or C0 % ck:
        return False
    if Cout == 32:
        return not bnr and not in_scale and pool_c0 == 0 and ((Wout % 32 == 0 and Hout % 8 == 0) or (Wout % 16 == 0 and Hout % 16 == 0))
    if Cout < 64 or Cout % 64:
        return False
    return hg_tile_pixels(Hout, Wout, Cout) != 0


def hg_shape(Hout, Wout, Cout):
    """(tile width, tile height, column block) launch_hg_t picks."""
    if Cout == 32:
        return (32, 8, 32) if Wout % 32 == 0 else (16, 16, 32)
    bn = 128 if Cout % 128 == 0 else 64
    if hg_tile_pixels(Hout, Wout, Cout) == 128:
        return 16, 8, bn
    return (32, 8, bn) if Wout % 32 == 0 else (16, 16, bn)


def halo_bnr_ok(C0, C1, Cout, out_ld, pool_c0=0, nchw=False, stats=False, bias=False, in_scale=False, epilogue=False, bnr_out=False):
    """conv_halo_bnr_ok for a shape the small-channel halo kernel takes (bnr_C = out_ld)."""
    persistent = C1 == 0 and C0 in (16, 32) and Cout <= 32
    return (persistent and not (in_scale or stats or epilogue or bias or nchw or bnr_out) and out_ld <= 32
            and out_ld <= (16 if Cout <= 16 else 32) and pool_c0 in (0, Cout))


def conv_kernel(dt, N, Hin, Win, Hout, Wout, C0, C1, Cout, R, out_mul, in_div, pad, has_out=True, nchw=False, stats=False,
                bias=False, in_scale=False, pool_c0=0, epilogue=False, bm32=2, bnr=False, bnr_out=False, bnr_mask=False, acc_src=False):
    """(family, profile name) of the kernel launch_conv picks.  Families: stem, hg_n32/64/128, halo_pm, halo_p, halo, igemm.
    bnr (ConvArgs::bnr_partial): the fused BatchNorm-backward reduction; a combination launch_conv refuses is an AssertionError."""
    Cin = C0 + C1
    tdt = dt  # profile names spell the type this way
    geo = (C0, C1, Cout, R, out_mul, in_div, pad, Hin, Win, Hout, Wout)
    hg = hg_applicable(dt, *geo, has_out, nchw, in_scale, pool_c0, bnr)
    halo = halo_applicable(*geo)
    if bnr_mask or acc_src:
        assert hg, "bnr_mask / acc_src: halo-GEMM only"
    if bnr_mask:
        assert bnr, "bnr_mask needs bnr_partial"
    if bnr:
        assert Hout % 2 == 0 and Wout % 2 == 0
        assert hg or (halo and halo_bnr_ok(C0, C1, Cout, pool_c0 or Cout, pool_c0, nchw, stats, bias, in_scale, epilogue, bnr_out)), \
            "fused reduction: halo-GEMM or the persistent small-channel kernel only"
    if in_scale:
        assert hg or halo, "lazy input: halo-GEMM or small-channel halo kernel only"
    kstep = 32 if dt == "f32" else 64
    if (not in_scale and dt == "bf16" and R == 7 and out_mul == 2 and in_div == 1 and pad == 3 and C0 == 8 and C1 == 0 and Cout == 64
            and has_out and not nchw and Hin == 2 * Hout and Win == 2 * Wout and Hout % 8 == 0 and Wout % 16 == 0
            and _rup(R * R * Cin, kstep) >= 8 * 4 * 13):
        return "stem", "conv_stem_bf16"
    if hg:
        bn = hg_shape(Hout, Wout, Cout)[2]
        return f"hg_n{bn}", f"conv3x3_hg_{tdt}_n{bn}"
    if halo:
        name = f"conv3x3_halo_{tdt}_ck{16 if Cin == 16 else 32}"
        if dt == "bf16" and C1 == 0 and C0 == 32 and Cout == 128 and not nchw and pool_c0 % 32 == 0 and not stats and not epilogue and not bias:
            return "halo_pm", name
        if C1 == 0 and Cin in (16, 32) and Cout <= 32:
            return "halo_p", name
        return "halo", name
    bn = _pick_bn(Cout)
    M = N * Hout * Wout
    ch = 4 if dt == "f32" else 8
    small = (not stats and bn >= 64 and _rup(R * R * Cin, kstep) >= 8 * 8 * ch and _cdiv(M, 128) * _cdiv(Cout, bn) < 256 and bm32)
    if small and bm32 >= 2 and _cdiv(M, 32) * _cdiv(Cout, bn) < 512:
        bn = 32
    tile = {128: "128x128", 64: "128x64", 32: "256x32", 16: "256x16"}[bn]
    return ("igemm_bm32" if small else "igemm"), f"conv_igemm_{tdt}_{tile}"


def wgrad_kernel(dt, N, Hin, Win, Hout, Wout, C0, C1, Cout, R, stride, pad, dy_ld=None, in_scale=False, dbias=False):
    """(family, profile name, geometry dict) of the kernel launch_wgrad picks.  Families: stem, big_kg1, big_kg2, halo, plain."""
    Cin = C0 + C1
    dy_ld = dy_ld or Cout
    same = R == 3 and stride == 1 and pad == 1 and Hout == Hin and Wout == Win
    # wg_big_geom
    ck = 32 if dt == "f32" else 64
    co = 64 if dt == "f32" else 128
    kg = 1
    if Cout % co:
        co //= 2
        kg = 2
    big = same and Hin % 8 == 0 and Win % 16 == 0 and Cin % ck == 0 and C0 % ck == 0 and Cout % co == 0 and dy_ld == Cout
    # wg_halo_geom
    CK = 16 if (Cin == 16 and C1 == 0) else 32 if (Cin % 32 == 0 and C0 % 32 == 0 and Cin <= 256) else 0
    halo = same and Hin % 8 == 0 and Win % 32 == 0 and CK and Cout <= 64 and dy_ld % 16 == 0
    cout_pad = _rup(Cout, 16)
    CO = 32 if cout_pad % 32 == 0 else 16
    if dbias:
        assert halo and CK == 16 and CO == 16 and cout_pad == 16 and Cin == 16 and dy_ld == 16, "dbias: 16 -> <= 16 layers only"
        big = False
    stem = (dt == "bf16" and R == 7 and stride == 2 and pad == 3 and C0 == 8 and C1 == 0 and Cout == 64 and dy_ld == 64 and
            Hin == 2 * Hout and Win == 2 * Wout and Hout % 8 == 0 and Wout % 16 == 0)
    if stem and not in_scale and not dbias:
        return "stem", "wgrad_stem_bf16", {"ntiles": N * Hout * Wout // 128, "cap": 512, "step": 1}
    if big:
        name = "wgrad3x3_big_f32" if dt == "f32" else ("wgrad3x3_big_bf16" if kg == 1 else "wgrad3x3_big_bf16_co64")
        return f"big_kg{kg}", name, {"ntiles": N * Hin * Win // 128, "per": (Cin // ck) * (Cout // co), "step": 1}
    if halo:
        name = "wgrad3x3_halo_f32" if dt == "f32" else f"wgrad3x3_halo_bf16_ck{CK}"
        return "halo", name, {"ntiles": N * Hin * Win // 256, "per": (Cin // CK) * (cout_pad // CO), "step": 2}
    assert not in_scale and not dbias
    geo = wg_plan(dt, N * Hout * Wout, Cin, Cout, R)
    if dt == "f32":
        return "plain", "wgrad_f32_64x64", geo
    return "plain", ("wgrad_bf16_128x128" if (Cout >= 128 and R * R * Cin >= 128) else "wgrad_bf16_64x64"), geo


def wg_plan(dt, M, Cin, Cout, R):
    """wg_plan and launch_wgrad_reduce of the gather-form weight gradient (wgrad.hip): the split count over the M output pixels, the
    pixels per split and of the last one, and the reduce kernel: its EL (elements per workgroup row), its grid and the passes a
    workgroup makes over the gradient (the grid is capped at 8 192 workgroups for EL = 64)."""
    Kg = R * R * Cin
    b = 128 if (dt == "bf16" and Cout >= 128 and Kg >= 128) else 64
    tiles = (_rup(Cout, b) // b) * (_rup(Kg, b) // b)
    want = max(1, min(_cdiv(768, tiles), max(1, _cdiv(M, 64 * 8))))
    pps = _rup(_cdiv(M, want), 64)
    splits = _cdiv(M, pps)
    total = Cout * Kg
    el = 16 if (splits >= 64 and total <= 65536) else 64
    grid = _cdiv(total, el) if el == 16 else min(_cdiv(total, 64), 8192)
    return {"splits": splits, "pps": pps, "last": M - (splits - 1) * pps, "reduce_el": el, "reduce_grid": grid, "reduce_total": total}


def tiles_per_workgroup(ntiles, grid):
    """(most, fewest) tiles a workgroup of a persistent grid walks: workgroup b takes tiles b, b + grid, b + 2 grid, ..."""
    grid = min(grid, ntiles)
    return _cdiv(ntiles, grid), (ntiles - (grid - 1) + grid - 1) // grid


def split_count(budget, per, ntiles):
    """nsplit of wg_halo_geom / wg_big_geom: budget workgroups shared by `per` channel-block pairs."""
    return max(1, min(budget // per, ntiles))


# ------------------------------------------------------------------------------------------------ convolution cases
@dataclass(frozen=True)
class ConvCase:
    name: str
    N: int
    H: int            # logical input extent (after the upsample of x0)
    W: int
    C0: int
    Cout: int
    C1: int = 0
    up0: bool = False
    R: int = 3
    stride: int = 1
    pad: int = 1
    bias: bool = False
    nchw: bool = False
    stats: bool = True
    backward: bool = True       # dx and dw through flair_conv2d_backward (single source only)
    need_dx: bool = True
    density: float = 0.5
    dtypes: tuple = DTYPES
    tune: tuple = ()            # ((switch, value), ...)
    fwd: object = field(default=None, compare=False)   # intended family: a string, or {"f32": ..., "bf16": ...}
    dx: object = field(default=None, compare=False)
    dw: object = field(default=None, compare=False)
    loops: tuple = ()           # which of "fwd", "dx", "dw" must walk more than one tile per workgroup, unevenly
    real_cin: int = 0           # channels beyond this are zero padding (the stem: 5 of 8)

    @property
    def Cin(self):
        return self.C0 + self.C1

    @property
    def Ho(self):
        return (self.H + 2 * self.pad - self.R) // self.stride + 1

    @property
    def Wo(self):
        return (self.W + 2 * self.pad - self.R) // self.stride + 1

    def tuned(self, key):
        return dict(self.tune).get(key, TUNE_DEFAULTS[key])

    def want(self, which, dt):
        v = getattr(self, which)
        return v[dt] if isinstance(v, dict) else v

    def fwd_kernel(self, dt):
        has_out = self.Cout % 8 == 0
        return conv_kernel(dt, self.N, self.H, self.W, self.Ho, self.Wo, self.C0, self.C1, self.Cout, self.R, self.stride, 1, self.pad,
                           has_out=has_out, nchw=self.nchw or not has_out, stats=self.stats, bias=self.bias,
                           bm32=self.tuned("FLAIR_IGEMM_BM32"))

    def dx_kernel(self, dt):
        return conv_kernel(dt, self.N, self.Ho, self.Wo, self.H, self.W, self.Cout, 0, self.Cin, self.R, 1, self.stride,
                           self.R - 1 - self.pad, bm32=self.tuned("FLAIR_IGEMM_BM32"))

    def dw_kernel(self, dt):
        return wgrad_kernel(dt, self.N, self.H, self.W, self.Ho, self.Wo, self.Cin, 0, self.Cout, self.R, self.stride, self.pad)

    def loop_shape(self, which, dt, per_cu=None):
        """(ntiles, grid) of the persistent launch of pass `which`; per_cu: resident workgroups per CU where the runtime decides."""
        if which == "dw":
            fam, _, g = self.dw_kernel(dt)
            if fam == "stem":
                return g["ntiles"], min(g["ntiles"], g["cap"])
            budget = self.tuned("FLAIR_WG_CUS_OP") if fam.startswith("big") else (self.tuned("FLAIR_WGH_WGS") or 256 * (per_cu or 1))
            return g["ntiles"], split_count(budget, g["per"], g["ntiles"])
        fam, _ = self.fwd_kernel(dt) if which == "fwd" else self.dx_kernel(dt)
        M = self.N * (self.Ho * self.Wo if which == "fwd" else self.H * self.W)
        if fam == "stem":
            return M // 128, min(M // 128, 512)
        assert fam in ("halo_p", "halo_pm"), fam
        cap = self.tuned("FLAIR_HALO_P_WGS") if fam == "halo_p" else 0
        return M // 256, min(M // 256, 256 * (cap or per_cu or 1))


_CAP = (("FLAIR_HALO_P_WGS", 1),)    # persistent small-channel grid = 256 workgroups whatever the runtime reports

CONV_CASES = [
    # ---- 1. persistent small-channel kernels (8x32 tiles; A/B register sets, prefetch two grids ahead)
    #         grid capped at 256: 288 tiles -> 2 and 1 per workgroup, 640 -> 3 and 2, 864 -> 4 and 3
    ConvCase("p16to16_288tiles", 3, 96, 256, 16, 16, nchw=True, density=0.25, tune=_CAP + (("FLAIR_WGH_WGS", 7),),
             fwd="halo_p", dx="halo_p", dw="halo", loops=("fwd", "dx", "dw")),
    ConvCase("p16to13_head_640tiles", 5, 128, 256, 16, 13, bias=True, nchw=True, stats=False, backward=False, tune=_CAP,
             fwd="halo_p", loops=("fwd",)),
    ConvCase("p32to16_640tiles", 5, 128, 256, 32, 16, density=0.25, tune=_CAP + (("FLAIR_WGH_WGS", 7),),
             fwd="halo_p", dx="halo_p", dw="halo", loops=("fwd", "dx", "dw")),
    ConvCase("p32to32_864tiles", 3, 256, 288, 32, 32, density=0.25, tune=_CAP + (("FLAIR_WGH_WGS", 5), ("FLAIR_WG_CUS_OP", 5)),
             fwd={"f32": "hg_n32", "bf16": "halo_p"}, dx={"f32": "hg_n32", "bf16": "halo_p"}, dw={"f32": "big_kg2", "bf16": "halo"},
             loops=("fwd", "dx", "dw")),
    ConvCase("p16to16_864tiles", 3, 256, 288, 16, 16, density=0.25, tune=_CAP + (("FLAIR_WGH_WGS", 5),),
             fwd="halo_p", dx="halo_p", dw="halo", loops=("fwd", "dx", "dw")),
    ConvCase("p16to32_288tiles", 3, 96, 256, 16, 32, density=0.25, tune=_CAP + (("FLAIR_WGH_WGS", 5),),
             fwd="halo_p", dx="halo_p", dw="halo", loops=("fwd", "dx", "dw")),
    # layer-sized, default grids (256 x the resident count the runtime reports)
    ConvCase("p16to16_512x512_default_grid", 2, 512, 512, 16, 16, density=0.25, fwd="halo_p", dx="halo_p", dw="halo"),
    # bf16 32 -> 128: the multi-block persistent kernel (no statistics / bias / NCHW copy); 2 112 tiles loop unevenly on 256, 512,
    # 768 and 1 024 workgroups.  fp32 takes the register-staged halo-GEMM.
    ConvCase("pm32to128_2112tiles", 3, 512, 352, 32, 128, stats=False, backward=False,
             fwd={"f32": "hg_n128", "bf16": "halo_pm"}, loops=("fwd",)),
    # the same layer WITH statistics runs one workgroup per tile (1 056 of them: more than any persistent grid of that shape)
    ConvCase("t32to128_stats_1056tiles", 3, 256, 352, 32, 128, density=0.25, backward=False, fwd={"f32": "hg_n128", "bf16": "halo"}),
    # ---- 2. small-channel weight gradient with nsplit < ntiles and a remainder (and the forward / data gradient of the shape)
    ConvCase("w64to32_23tiles", 1, 184, 32, 64, 32, tune=(("FLAIR_WGH_WGS", 14), ("FLAIR_WG_CUS_OP", 10)),
             fwd="hg_n32", dx={"f32": "hg_n64", "bf16": "halo"}, dw={"f32": "big_kg2", "bf16": "halo"}, loops=("dw",)),
    ConvCase("w128to32_23tiles", 1, 184, 32, 128, 32, tune=(("FLAIR_WGH_WGS", 20), ("FLAIR_WG_CUS_OP", 20)),
             fwd="hg_n32", dx={"f32": "hg_n128", "bf16": "halo_pm"}, dw={"f32": "big_kg2", "bf16": "halo"}, loops=("dw",)),
    ConvCase("w32to64_23tiles", 1, 184, 32, 32, 64, tune=(("FLAIR_WGH_WGS", 10), ("FLAIR_WG_CUS_OP", 5)),
             fwd={"f32": "hg_n64", "bf16": "halo"}, dx="hg_n32", dw={"f32": "big_kg1", "bf16": "halo"}, loops=("dw",)),
    # ---- 3. large weight gradient (8x16 tiles), both kg values, one and several input-channel blocks; 4. halo-GEMM tile shapes
    #         with nwork >= 9 and nwork % 8 != 0 (XCD remap with q > 0 and r > 0)
    ConvCase("hg64to128_16x8_nwork15", 1, 40, 48, 64, 128, tune=(("FLAIR_WG_CUS_OP", 8),),
             fwd="hg_n128", dx="hg_n64", dw="big_kg1", loops=("dw",)),
    ConvCase("hg128to64_16x8_nwork15", 1, 40, 48, 128, 64, tune=(("FLAIR_WG_CUS_OP", 8),),
             fwd="hg_n64", dx="hg_n128", dw={"f32": "big_kg1", "bf16": "big_kg2"}, loops=("dw",)),
    ConvCase("hg128to128_16x8_nwork9", 1, 24, 48, 128, 128, tune=(("FLAIR_WG_CUS_OP", 16),),
             fwd="hg_n128", dx="hg_n128", dw="big_kg1", loops=("dw",)),
    ConvCase("hg64to64_32x8_nwork9", 1, 24, 96, 64, 64, tune=(("FLAIR_WG_CUS_OP", 8),),
             fwd="hg_n64", dx="hg_n64", dw={"f32": "big_kg1", "bf16": "big_kg2"}, loops=("dw",)),
    ConvCase("hg128to192_16x16_nwork27", 1, 48, 48, 128, 192, tune=(("FLAIR_WG_CUS_OP", 60),),
             fwd="hg_n64", dx="hg_n128", dw={"f32": "big_kg1", "bf16": "big_kg2"}, loops=("dw",)),
    ConvCase("hg128to32_32x8_nwork9", 1, 24, 96, 128, 32, backward=False, fwd="hg_n32"),
    ConvCase("hg64up64to32_16x16_nwork9", 1, 48, 48, 64, 32, C1=64, up0=True, backward=False, fwd="hg_n32"),
    ConvCase("hg128up64to128_16x8_nwork9", 1, 24, 48, 128, 128, C1=64, up0=True, backward=False, fwd="hg_n128"),
    ConvCase("hg512to128_16x8_nwork9", 1, 24, 48, 512, 128, density=0.25, tune=(("FLAIR_WG_CUS_OP", 64),),
             fwd="hg_n128", dx="hg_n128", dw="big_kg1", loops=("dw",)),
    # ---- 5. gather-form kernel: stride 2, 1x1, ragged channel counts, pixel counts off the 128 / 256-row block
    ConvCase("g3x3s2_64to128_240px", 1, 24, 40, 64, 128, stride=2, fwd="igemm", dx="igemm_bm32", dw="plain"),
    ConvCase("g3x3s2_64to128_240px_bm32_1", 1, 24, 40, 64, 128, stride=2, stats=False, tune=(("FLAIR_IGEMM_BM32", 1),),
             fwd="igemm_bm32", dx="igemm_bm32", dw="plain"),
    ConvCase("g3x3s2_64to128_240px_bm32_0", 1, 24, 40, 64, 128, stride=2, stats=False, tune=(("FLAIR_IGEMM_BM32", 0),),
             fwd="igemm", dx="igemm", dw="plain"),
    ConvCase("g1x1s2_128to256_105px", 3, 10, 14, 128, 256, R=1, stride=2, pad=0, fwd="igemm", dx={"f32": "igemm_bm32", "bf16": "igemm"}, dw="plain"),
    ConvCase("g3x3_16to13_bias_nchw_240px", 1, 12, 20, 16, 13, bias=True, nchw=True, stats=False, backward=False, fwd="igemm"),
    ConvCase("g3x3_64to192_120px", 1, 10, 12, 64, 192, nchw=True, fwd="igemm", dx="igemm_bm32", dw="plain"),
    ConvCase("g3x3_32to16_nontileable", 2, 20, 24, 32, 16, fwd="igemm", dx="igemm", dw="plain"),
    # the gather-form weight gradient past one or two splits (WG_PLAN_WANT below has the numbers): 14 splits of 512 pixels, the last
    # with 256, reduced by wgrad_reduce_kernel<64> in its four-way loop (slab groups 0 and 1) and its remainder loop (2 and 3);
    # 66 splits of a 2 304-element gradient: wgrad_reduce_kernel<16>; a 1 179 648-element gradient: the reduce grid at its 8 192-block
    # cap, three passes, the last one ragged
    ConvCase("g3x3s2_64to128_14splits", 3, 96, 96, 64, 128, stride=2, fwd="igemm", dx="igemm_bm32", dw="plain"),
    ConvCase("g3x3_16to16_w48_66splits", 1, 704, 48, 16, 16, density=0.25, fwd="igemm", dx="igemm", dw="plain"),
    ConvCase("g3x3s2_256to512_reduce_cap", 1, 8, 8, 256, 512, stride=2, density=0.25, fwd="igemm", dx="igemm_bm32", dw="plain"),
    # 7x7 stride-2 stem, 5 real channels of 8: fp32 gather form, bf16 direct kernels (8x16 tiles, 512 persistent workgroups:
    # 560 tiles -> 2 and 1 per workgroup)
    ConvCase("stem_560tiles", 5, 256, 224, 8, 64, R=7, stride=2, pad=3, need_dx=False, real_cin=5,
             fwd={"f32": "igemm", "bf16": "stem"}, dw={"f32": "plain", "bf16": "stem"}, loops=("fwd", "dw")),
    ConvCase("stem_36tiles", 3, 64, 96, 8, 64, R=7, stride=2, pad=3, need_dx=False, real_cin=5,
             fwd={"f32": "igemm", "bf16": "stem"}, dw={"f32": "plain", "bf16": "stem"}),
    ConvCase("stem_18x20_gather_form", 2, 36, 40, 8, 64, R=7, stride=2, pad=3, need_dx=False, real_cin=5, fwd="igemm", dw="plain"),
]


# name -> (splits, pixels per split, pixels of the last split, reduce EL, reduce grid), both dtypes alike
WG_PLAN_WANT = {
    "g3x3s2_64to128_14splits": (14, 512, 256, 64, 1152),
    "g3x3_16to16_w48_66splits": (66, 512, 512, 16, 144),
    "g3x3s2_256to512_reduce_cap": (1, 64, 16, 64, 8192),
}
WG_ACCUMULATE_CASE = "g3x3s2_64to128_14splits"     # run again through conv2d_wgrad_ex(dw=prefilled, accumulate=True)


def check_wg_plan(c):
    """The gather-form weight gradient of the case splits and reduces as the table says (asserted on the restated wg_plan)."""
    for dt in c.dtypes:
        fam, _, g = c.dw_kernel(dt)
        assert fam == "plain", (c.name, dt, fam)
        got = (g["splits"], g["pps"], g["last"], g["reduce_el"], g["reduce_grid"])
        assert got == WG_PLAN_WANT[c.name], (c.name, dt, got)
        if g["reduce_el"] == 64 and g["splits"] > 1:     # G = 4 slab groups: the four-way loop runs where z + 12 < splits
            four = [zg for zg in range(4) if zg + 12 < g["splits"]]
            assert four and len(four) < 4, (c.name, "both loops of wgrad_reduce_kernel<64>")
        if g["reduce_grid"] == 8192:
            blocks = _cdiv(g["reduce_total"], 64)
            assert blocks > 2 * 8192 and blocks % 8192, (c.name, "ragged last pass", blocks)


def case_inputs(c):
    """Seeded ternary x0 (stored extent), x1, w, bias, dy (all fp32 CPU, NCHW / OIHW)."""
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in c.name))
    h0, w0 = (c.H // 2, c.W // 2) if c.up0 else (c.H, c.W)
    x0 = ternary((c.N, c.C0, h0, w0), g, c.density)
    x1 = ternary((c.N, c.C1, c.H, c.W), g, c.density) if c.C1 else None
    if c.real_cin:
        x0[:, c.real_cin:] = 0
    w = ternary((c.Cout, c.Cin, c.R, c.R), g, c.density)
    if c.real_cin:
        w[:, c.real_cin:] = 0
    b = ints((c.Cout,), g, -3, 3) if c.bias else None
    dy = ternary((c.N, c.Cout, c.Ho, c.Wo), g, c.density) if c.backward else None
    return x0, x1, w, b, dy


def assemble_input(x0, x1, up0):
    xin = F.interpolate(x0, scale_factor=2, mode="nearest") if up0 else x0
    return torch.cat([xin, x1], 1) if x1 is not None else xin


@functools.lru_cache(maxsize=2)
def case_reference(c):
    """fp64 CPU reference of one case (shared by both dtypes): dict with x0, x1, w, b, dy and y, s1, s2, dx, dw."""
    x0, x1, w, b, dy = case_inputs(c)
    xin = assemble_input(x0, x1, c.up0).double()
    wd = w.double()
    y = F.conv2d(xin, wd, None if b is None else b.double(), stride=c.stride, padding=c.pad)
    ref = {"x0": x0, "x1": x1, "w": w, "b": b, "dy": dy, "y": y, "s1": y.sum(dim=(0, 2, 3)), "s2": (y * y).sum(dim=(0, 2, 3)),
           "sabs": y.abs().sum(dim=(0, 2, 3)), "dx": None, "dw": None}
    if c.backward:
        dyd = dy.double()
        if c.need_dx:
            ref["dx"] = torch.nn.grad.conv2d_input(xin.shape, wd, dyd, stride=c.stride, padding=c.pad)
        ref["dw"] = torch.nn.grad.conv2d_weight(xin, wd.shape, dyd, stride=c.stride, padding=c.pad)
        ref["dw_terms"] = c.N * c.Ho * c.Wo   # every term of a weight-gradient sum is in {-1, 0, 1}
    return ref


def check_exact_range(c, ref):
    """The case is inside the exact range: asserted on the reference alone.  A case outside it is a failure, never a skip."""
    assert float(ref["y"].abs().max()) <= 256, (c.name, "max |y|", float(ref["y"].abs().max()))
    if c.stats:
        assert float(ref["s2"].max()) < EXACT, (c.name, "max_c sum y^2", float(ref["s2"].max()))
        assert float(ref["sabs"].max()) < EXACT, (c.name, "max_c sum |y|", float(ref["sabs"].max()))
    if ref["dx"] is not None:
        assert float(ref["dx"].abs().max()) <= 256, (c.name, "max |dx|", float(ref["dx"].abs().max()))
    if ref["dw"] is not None:
        assert float(ref["dw"].abs().max()) < EXACT and ref["dw_terms"] < EXACT, (c.name, "dw")


def check_dispatch_and_loops(c):
    """The restated dispatch sends the case where it is meant to go, and the looping cases loop: more than one tile per workgroup,
    unevenly (plain integer arithmetic, the launcher's own)."""
    out = {}
    for dt in c.dtypes:
        assert c.fwd_kernel(dt)[0] == c.want("fwd", dt), (c.name, dt, "fwd", c.fwd_kernel(dt))
        if c.backward:
            if c.need_dx:
                assert c.dx_kernel(dt)[0] == c.want("dx", dt), (c.name, dt, "dx", c.dx_kernel(dt))
            assert c.dw_kernel(dt)[0] == c.want("dw", dt), (c.name, dt, "dw", c.dw_kernel(dt)[:2])
        for which in c.loops:
            fam = (c.fwd_kernel(dt) if which == "fwd" else c.dx_kernel(dt) if which == "dx" else c.dw_kernel(dt))[0]
            if fam not in ("halo_p", "halo_pm", "stem", "halo", "big_kg1", "big_kg2"):
                continue   # (the other dtype's kernel of this shape is not a persistent one)
            if which == "dw" and fam == "halo" and not c.tuned("FLAIR_WGH_WGS"):
                continue
            runtime_decides = fam == "halo_pm" or (fam == "halo_p" and not c.tuned("FLAIR_HALO_P_WGS"))
            for per_cu in ((1, 2, 3, 4) if runtime_decides else (None,)):
                ntiles, grid = c.loop_shape(which, dt, per_cu)
                most, fewest = tiles_per_workgroup(ntiles, grid)
                assert grid < ntiles and ntiles % grid and most > fewest >= 1, (c.name, dt, which, ntiles, grid)
                out[(dt, which, per_cu)] = (ntiles, grid, most, fewest)
    return out


# ------------------------------------------------------------------------------------------------ fused forms (flair_conv2d_ex / _wgrad_ex)
@dataclass(frozen=True)
class FusedCase:
    name: str
    kind: str          # lazy | epilogue | accumulate | acc_src | pool | argmax | wgrad2 | wgrad_lazy | dbias
    N: int
    H: int
    W: int
    C0: int
    Cout: int
    C1: int = 0
    up0: bool = False
    pool_c0: int = 0
    skip_accumulate: bool = False
    density: float = 0.5
    tune: tuple = ()
    kernel: object = field(default=None, compare=False)      # intended family of the launch (string or per-dtype dict)
    loops: bool = False

    @property
    def mode(self):   # the gradient-side options are exercised as the network uses them: on a stride-1 data gradient
        return 1 if self.kind in ("accumulate", "acc_src", "pool") else 0

    def tuned(self, key):
        return dict(self.tune).get(key, TUNE_DEFAULTS[key])

    def want(self, dt):
        return self.kernel[dt] if isinstance(self.kernel, dict) else self.kernel


FUSED_CASES = [
    # lazy BatchNorm + ReLU on the input: padding pixels stay zero whatever the shift
    FusedCase("lazy_p16to16_small", "lazy", 1, 16, 64, 16, 16, kernel="halo_p"),
    FusedCase("lazy_p32to32_640tiles", "lazy", 5, 128, 256, 32, 32, density=0.25, tune=_CAP, kernel="halo_p", loops=True),
    FusedCase("lazy_hg64to64_nwork9", "lazy", 1, 24, 96, 64, 64, density=0.25, kernel="hg_n64"),
    FusedCase("lazy_hg128to128_nwork15", "lazy", 1, 40, 48, 128, 128, density=0.25, kernel="hg_n128"),
    # two chunks of 32 channels into one 32-wide block: the plain small-channel kernel (the halo-GEMM has no lazy 32-wide flavour)
    FusedCase("lazy_halo64to32_1tile", "lazy", 1, 8, 32, 64, 32, density=0.25, kernel="halo"),
    FusedCase("wlazy_p16to16_small", "wgrad_lazy", 1, 16, 64, 16, 16, kernel="halo"),
    FusedCase("wlazy_p32to16_23tiles", "wgrad_lazy", 1, 184, 32, 32, 16, tune=(("FLAIR_WGH_WGS", 10),), kernel="halo", loops=True),
    FusedCase("wlazy_big64to64_15tiles", "wgrad_lazy", 1, 40, 48, 64, 64, tune=(("FLAIR_WG_CUS_OP", 4),),
              kernel={"f32": "big_kg1", "bf16": "big_kg2"}, loops=True),
    # inference epilogue relu(acc * oscale + oshift + bias + ores)
    FusedCase("epi_p16to16_small", "epilogue", 1, 16, 64, 16, 16, density=0.25, kernel="halo_p"),
    FusedCase("epi_p32to32_640tiles", "epilogue", 5, 128, 256, 32, 32, density=0.25, tune=_CAP, kernel={"f32": "hg_n32", "bf16": "halo_p"}, loops=True),
    FusedCase("epi_p32to16_640tiles", "epilogue", 5, 128, 256, 32, 16, density=0.25, tune=_CAP, kernel="halo_p", loops=True),
    FusedCase("epi_hg64to128_nwork15", "epilogue", 1, 40, 48, 64, 128, density=0.25, kernel="hg_n128"),
    FusedCase("epi_igemm_64to64_120px", "epilogue", 1, 10, 12, 64, 64, density=0.25, kernel="igemm_bm32"),
    # accumulate into a pre-filled output / addend from a third tensor
    FusedCase("acc_p16to16_small", "accumulate", 1, 16, 64, 16, 16, kernel="halo_p"),
    FusedCase("acc_p32to16_640tiles", "accumulate", 5, 128, 256, 32, 16, density=0.25, tune=_CAP, kernel="halo_p", loops=True),
    FusedCase("acc_hg128to64_nwork15", "accumulate", 1, 40, 48, 128, 64, kernel="hg_n64"),
    FusedCase("accsrc_hg64to64_nwork9", "acc_src", 1, 24, 96, 64, 64, kernel="hg_n64"),
    FusedCase("accsrc_hg128to128_nwork15", "acc_src", 1, 40, 48, 128, 128, kernel="hg_n128"),
    # fused backward of "nearest x2 upsample ++ skip": first pool_c0 columns 2x2 sum-pooled, the rest to out_skip
    FusedCase("pool_p16to32_all_small", "pool", 1, 16, 64, 16, 32, pool_c0=32, kernel="halo_p"),
    FusedCase("pool_p32to32_all_640tiles", "pool", 5, 128, 256, 32, 32, pool_c0=32, density=0.25, tune=_CAP, kernel="halo_p", loops=True),
    FusedCase("pool_t32to96_c32_288tiles", "pool", 3, 96, 256, 32, 96, pool_c0=32, density=0.25, kernel="halo"),
    FusedCase("pool_t32to96_c64_skipacc", "pool", 1, 16, 64, 32, 96, pool_c0=64, skip_accumulate=True, kernel="halo"),
    FusedCase("pool_hg64to192_c128", "pool", 1, 48, 48, 64, 192, pool_c0=128, kernel="hg_n64"),
    FusedCase("pool_hg64to192_c64_skipacc", "pool", 1, 48, 48, 64, 192, pool_c0=64, skip_accumulate=True, kernel="hg_n64"),
    FusedCase("pool_hg64to128_all", "pool", 1, 40, 48, 64, 128, pool_c0=128, kernel="hg_n128"),
    # argmax epilogue of the head: integer logits, ties in most pixels
    FusedCase("argmax_p16to13_small", "argmax", 1, 16, 64, 16, 13, density=0.25, kernel="halo_p"),
    FusedCase("argmax_p16to19_640tiles", "argmax", 5, 128, 256, 16, 19, density=0.25, tune=_CAP, kernel="halo_p", loops=True),
    # two-source weight gradient, with and without the upsample of the first
    FusedCase("wg2_up_64x64to32_23tiles", "wgrad2", 1, 184, 32, 64, 32, C1=64, up0=True, tune=(("FLAIR_WGH_WGS", 20), ("FLAIR_WG_CUS_OP", 20)),
              kernel={"f32": "big_kg2", "bf16": "halo"}, loops=True),
    FusedCase("wg2_32x32to16_small", "wgrad2", 1, 16, 64, 32, 16, C1=32, kernel="halo"),
    FusedCase("wg2_up_128x64to128_15tiles", "wgrad2", 1, 40, 48, 128, 128, C1=64, up0=True, tune=(("FLAIR_WG_CUS_OP", 24),),
              kernel="big_kg1", loops=True),
    # bias gradient folded into the 16 -> <= 16 weight-gradient kernel
    FusedCase("dbias_16to16_small", "dbias", 1, 16, 64, 16, 16, kernel="halo"),
    FusedCase("dbias_16to13_288tiles", "dbias", 3, 96, 256, 16, 13, tune=(("FLAIR_WGH_WGS", 7),), kernel="halo", loops=True),
]


def fused_kernel(c, dt):
    """(family, profile name[, geometry]) of the launch a fused case makes."""
    if c.kind in ("wgrad2", "wgrad_lazy", "dbias"):
        return wgrad_kernel(dt, c.N, c.H, c.W, c.H, c.W, c.C0, c.C1, c.Cout, 3, 1, 1, dy_ld=_rup(c.Cout, 16) if c.kind == "dbias" else None,
                            in_scale=c.kind == "wgrad_lazy", dbias=c.kind == "dbias")
    has_out = c.kind != "argmax"
    return conv_kernel(dt, c.N, c.H, c.W, c.H, c.W, c.C0, c.C1, c.Cout, 3, 1, 1, 1, has_out=has_out, in_scale=c.kind == "lazy",
                       pool_c0=c.pool_c0, epilogue=c.kind == "epilogue", bias=c.kind in ("epilogue", "argmax"))


@functools.lru_cache(maxsize=2)
def fused_reference(c):
    """Inputs (fp32 CPU) and the fp64 expectation of one fused case."""
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in c.name))
    N, H, W, Cin = c.N, c.H, c.W, c.C0 + c.C1
    h0, w0 = (H // 2, W // 2) if c.up0 else (H, W)
    r = {"x0": ternary((N, c.C0, h0, w0), g, c.density), "x1": ternary((N, c.C1, H, W), g, c.density) if c.C1 else None}
    xin = assemble_input(r["x0"], r["x1"], c.up0).double()
    if c.kind in ("wgrad2", "wgrad_lazy", "dbias"):
        ld = _rup(c.Cout, 16) if c.kind == "dbias" else c.Cout
        dy = ternary((N, ld, H, W), g, c.density)
        dy[:, c.Cout:] = 0
        r["dy"] = dy
        if c.kind == "wgrad_lazy":
            r["in_scale"], r["in_shift"] = ints((Cin,), g, 1, 2), ints((Cin,), g, -1, 1)
            xin = torch.relu(xin * r["in_scale"].double().view(1, -1, 1, 1) + r["in_shift"].double().view(1, -1, 1, 1))
        r["dw"] = torch.nn.grad.conv2d_weight(xin, (c.Cout, Cin, 3, 3), dy[:, :c.Cout].double(), padding=1)
        r["dbias"] = dy[:, :c.Cout].double().sum(dim=(0, 2, 3))
        r["terms"] = 3 * N * H * W   # |x'| <= 3 with scale <= 2 and shift <= 1
        return r
    # mode 1: the weights are the forward layer's [Cin][Cout][3][3] and the result its stride-1 data gradient
    r["w"] = ternary((Cin, c.Cout, 3, 3) if c.mode == 1 else (c.Cout, Cin, 3, 3), g, c.density)
    wd = r["w"].double()
    if c.kind == "lazy":
        r["in_scale"], r["in_shift"] = ints((Cin,), g, 1, 2), ints((Cin,), g, -1, 1)
        xin = torch.relu(xin * r["in_scale"].double().view(1, -1, 1, 1) + r["in_shift"].double().view(1, -1, 1, 1))
    # (zero padding AFTER the lazy transform: pixels outside the image stay zero)
    acc = F.conv_transpose2d(xin, wd, padding=1) if c.mode == 1 else F.conv2d(xin, wd, padding=1)
    r["acc"] = acc
    if c.kind == "lazy":
        r["y"] = acc
        r["s1"], r["s2"], r["sabs"] = acc.sum(dim=(0, 2, 3)), (acc * acc).sum(dim=(0, 2, 3)), acc.abs().sum(dim=(0, 2, 3))
    elif c.kind == "epilogue":
        r["oscale"], r["oshift"], r["bias"] = ints((c.Cout,), g, -2, 2), ints((c.Cout,), g, -3, 3), ints((c.Cout,), g, -3, 3)
        r["ores"] = ints((N, c.Cout, H, W), g, -4, 4)
        v = lambda t: t.double().view(1, -1, 1, 1)
        r["pre"] = acc * v(r["oscale"]) + v(r["oshift"]) + v(r["bias"]) + r["ores"].double()
        r["y"] = torch.relu(r["pre"])
    elif c.kind in ("accumulate", "acc_src"):
        r["prev"] = ints((N, c.Cout, H, W), g, -8, 8)
        r["y"] = acc + r["prev"].double()
    elif c.kind == "pool":
        r["prev_skip"] = ints((N, c.Cout - c.pool_c0, H, W), g, -8, 8) if c.skip_accumulate else None
        r["y"] = F.avg_pool2d(acc[:, :c.pool_c0], 2) * 4
        r["skip"] = acc[:, c.pool_c0:] + (r["prev_skip"].double() if c.skip_accumulate else 0)
    elif c.kind == "argmax":
        r["bias"] = ints((c.Cout,), g, -1, 1)
        r["y"] = acc + r["bias"].double().view(1, -1, 1, 1)
        r["preds"] = torch.argmax(r["y"], dim=1)
        r["maxprob"] = torch.softmax(r["y"], dim=1).max(dim=1).values
    return r


def check_fused_range(c, r):
    if "dw" in r:
        assert float(r["dw"].abs().max()) < EXACT and r["terms"] < EXACT, (c.name, "dw")
        assert float(r["dbias"].abs().max()) < EXACT
        return
    for k in ("acc", "y", "pre", "skip"):
        if k in r and r[k].numel():
            assert float(r[k].abs().max()) <= 256, (c.name, "max |%s|" % k, float(r[k].abs().max()))
    if "s2" in r:
        assert float(r["s2"].max()) < EXACT and float(r["sabs"].max()) < EXACT, (c.name, "statistics")


def check_fused_dispatch_and_loops(c):
    out = {}
    for dt in DTYPES:
        k = fused_kernel(c, dt)
        assert k[0] == c.want(dt), (c.name, dt, k[:2])
        if not c.loops:
            continue
        if len(k) == 3:   # weight gradient
            budget = c.tuned("FLAIR_WG_CUS_OP") if k[0].startswith("big") else c.tuned("FLAIR_WGH_WGS")
            assert budget > 0
            ntiles, grid = k[2]["ntiles"], split_count(budget, k[2]["per"], k[2]["ntiles"])
        else:
            if k[0] != "halo_p":
                continue   # (fp32 sends this shape to a halo-GEMM kernel: one tile per workgroup)
            assert c.tuned("FLAIR_HALO_P_WGS") == 1
            ntiles, grid = c.N * c.H * c.W // 256, 256
        most, fewest = tiles_per_workgroup(ntiles, grid)
        assert grid < ntiles and ntiles % grid and most > fewest >= 1, (c.name, dt, ntiles, grid)
        out[dt] = (ntiles, min(grid, ntiles), most, fewest)
    return out


# ------------------------------------------------------------------------------------------------ reductions at their caps
BN_BLOCK_CAP, CE_BLOCK_CAP = 2048, 2048
BN_CASES = [(3, 383, 467, 16), (3, 383, 467, 64)]                 # N, H, W, C: 536 583 rows > 2 048 * 256, not a multiple of 256
POOL_CASES = [(3, 256, 256, 64), (5, 128, 96, 32)]                # N, H, W, C (odd N)
CE_SHAPES = [(9, 512, 512), (5, 37, 53), (3, 419, 421)]           # vec4 kernel past its cap; scalar kernel small / past the cap


def check_reduction_shapes():
    for N, H, W, C in BN_CASES:
        rows = N * H * W
        assert rows > BN_BLOCK_CAP * 256 and rows % 256 and rows < EXACT
    B, H, W = CE_SHAPES[0]
    assert (H * W) % 4 == 0 and B * H * W > CE_BLOCK_CAP * 256 * 4
    B, H, W = CE_SHAPES[1]
    assert (H * W) % 4 and B * H * W < CE_BLOCK_CAP * 256
    B, H, W = CE_SHAPES[2]
    assert (H * W) % 4 and B * H * W > CE_BLOCK_CAP * 256
    for N, H, W, C in POOL_CASES:
        assert N % 2 == 1 and H % 2 == 0 and W % 2 == 0
