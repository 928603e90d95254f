"""Case table and fp64 references of the exact operator tests of the U-Net step's fused backward forms
(test_gpu_bwd_fused_exact.py, test_bwd_fused_cases_cpu.py).

Same rules as exact_cases.py: data in {-1, 0, 1} (small integers for y, scale, shift, coefficients and addends), every expectation an
fp64 CPU computation (conv_transpose2d / autograd / plain indexing), the comparison torch.equal, and the exact-range conditions
asserted on the reference alone: sums of magnitudes below 2^24, bf16 outputs within +-256.  Every convolution case names the kernel
family it is written for and the restated dispatch of exact_cases (conv_kernel with its bnr arguments) must agree.
This module needs no device."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

import exact_cases as E
from exact_cases import DTYPES, EXACT, _CAP, _rup, ints, ternary

TOL = {"f32": 2e-4, "bf16": 3e-2}   # test_gpu_ops_exact.py's: what passes through a division by a row count that is no power of two


def _gen(name):
    return torch.Generator().manual_seed(sum(ord(ch) for ch in name))


def _v(t):
    return t.double().view(1, -1, 1, 1)


def mask_inputs(g, shape, from_out):
    """y in [-3, 3]; scale in {-1, 0, 1} and shift in {-1, 0, 1} per channel, every one of the nine pairs present (C >= 16);
    `out` in {0, 1, 2}, drawn independently of y, for the units whose mask is out > 0."""
    Cc = shape[1]
    y = ints(shape, g, -3, 3)
    pairs = torch.tensor([(a, b) for a in (1, -1, 0) for b in (-1, 0, 1)], dtype=torch.float32)
    sel = torch.arange(Cc) % 9
    sel = sel[torch.randperm(Cc, generator=g)]
    scale, shift = pairs[sel, 0].contiguous(), pairs[sel, 1].contiguous()
    out = ints(shape, g, 0, 2) if from_out else None
    m = (out.double() > 0) if from_out else (y.double() * _v(scale) + _v(shift) > 0)
    return y, scale, shift, out, m.double()


def check_mask_variety(name, y, scale, shift):
    """[y scale + shift > 0] is on in some channels, off in others, mixed in most, and zero and negative scales occur"""
    on = (y.double() * _v(scale) + _v(shift) > 0).double().mean(dim=(0, 2, 3))
    assert float(on.min()) == 0.0 and float(on.max()) == 1.0 and bool(((on > 0) & (on < 1)).any()), (name, "mask variety")
    assert bool((scale == 0).any()) and bool((scale < 0).any()), name


# ------------------------------------------------------------------------------------------------ a. BNR epilogue of the data gradient
@dataclass(frozen=True)
class BnrCase:
    name: str
    N: int
    H: int
    W: int
    C0: int            # channels of the incoming gradient (the forward layer's output)
    Cout: int          # channels of the data gradient
    from_out: bool = False       # bnr_out: mask = out > 0 (a unit with a residual branch)
    bnr_mask: bool = False       # store dz * m
    accumulate: bool = False
    acc_src: bool = False
    pool_c0: int = 0
    skip_accumulate: bool = False
    density: float = 0.5
    tune: tuple = ()
    kernel: object = field(default=None, compare=False)
    loops: bool = False

    def want(self, dt):
        return self.kernel[dt] if isinstance(self.kernel, dict) else self.kernel

    def tuned(self, key):
        return dict(self.tune).get(key, E.TUNE_DEFAULTS[key])

    @property
    def Cy(self):      # channels of `out`, y and the partial sums
        return self.pool_c0 or self.Cout

    def launch(self, dt):
        return E.conv_kernel(dt, self.N, self.H, self.W, self.H, self.W, self.C0, 0, self.Cout, 3, 1, 1, 1, pool_c0=self.pool_c0,
                             bnr=True, bnr_out=self.from_out, bnr_mask=self.bnr_mask, acc_src=self.acc_src)

    def grid_rows(self, dt):
        """conv_grid_rows of the launch: rows of the partial.  None where the runtime's occupancy decides (uncapped persistent grid)."""
        fam = self.launch(dt)[0]
        px = self.N * self.H * self.W
        if fam.startswith("hg_"):
            tw, th, _ = E.hg_shape(self.H, self.W, self.Cout)
            return px // (tw * th)
        assert fam == "halo_p", fam
        cap = self.tuned("FLAIR_HALO_P_WGS")
        if cap == 1:
            return min(px // 256, 256)
        return px // 256 if px // 256 <= 256 else None


BNR_CASES = [
    # 1. halo-GEMM, 64-wide column blocks, mask from y.  9 work items: XCD remap with q = 1, r = 1; 192 -> 192: three column blocks
    #    per tile (n0 = 0, 64, 128) on 32x8 tiles; the 16x16 and 16x8 tile variants of the 64-wide kernel get one shape each
    BnrCase("bnr_hg64to64_32x8_nwork9", 1, 24, 96, 64, 64, kernel="hg_n64"),
    BnrCase("bnr_hg192to192_32x8_n0", 1, 24, 32, 192, 192, density=0.25, kernel="hg_n64"),
    BnrCase("bnr_hg64to64_16x16_nwork9", 1, 48, 48, 64, 64, kernel="hg_n64"),
    BnrCase("bnr_hg128to64_16x8_nwork15", 1, 40, 48, 128, 64, density=0.25, kernel="hg_n64"),
    # 2. 128-wide: 15 work items on 16x8 tiles (the only tile shape launch_hg_t gives a 128-wide layer under the default switches:
    #    every shape that tiles by 256 pixels also tiles by 16x8); two column blocks in the second
    BnrCase("bnr_hg128to128_16x8_nwork15", 1, 40, 48, 128, 128, density=0.25, kernel="hg_n128"),
    BnrCase("bnr_hg64to256_16x8_n0", 1, 24, 48, 64, 256, kernel="hg_n128"),
    # 3. residual unit: mask from `out` (inconsistent with y on purpose), accumulated into a pre-filled gradient
    BnrCase("bnr_out_acc_hg64to64", 1, 24, 96, 64, 64, from_out=True, accumulate=True, kernel="hg_n64"),
    BnrCase("bnr_out_acc_mask_hg128to128", 1, 40, 48, 128, 128, from_out=True, accumulate=True, bnr_mask=True, density=0.25, kernel="hg_n128"),
    # 4. masked store + addend from a third tensor
    BnrCase("bnr_mask_accsrc_hg128to128", 1, 40, 48, 128, 128, bnr_mask=True, accumulate=True, acc_src=True, density=0.25, kernel="hg_n128"),
    BnrCase("bnr_mask_hg64to64", 1, 24, 96, 64, 64, bnr_mask=True, kernel="hg_n64"),
    # 5. pooled: y and the partial have the pooled shape; column blocks at n0 >= pool_c0 store skip columns and leave the partial
    #    (and, with bnr_mask, the values they store) alone
    BnrCase("bnr_pool_hg64to128_all", 1, 40, 48, 64, 128, pool_c0=128, kernel="hg_n128"),
    BnrCase("bnr_pool_hg64to192_c64_skipacc", 1, 48, 48, 64, 192, pool_c0=64, skip_accumulate=True, kernel="hg_n64"),
    BnrCase("bnr_pool_mask_hg64to192_c64", 1, 48, 48, 64, 192, pool_c0=64, bnr_mask=True, kernel="hg_n64"),
    BnrCase("bnr_pool_acc_hg64to128_c128", 1, 40, 48, 64, 128, pool_c0=128, accumulate=True, kernel="hg_n128"),
    # 6. persistent small-channel kernel: one partial row per WORKGROUP; 640 tiles on 256 workgroups: 3 and 2 tiles each.
    #    (fp32 32 -> 32 would go to the 32-wide halo-GEMM, which has no fused reduction: with bnr it stays here in both dtypes)
    BnrCase("bnr_p16to16_small", 1, 16, 64, 16, 16, kernel="halo_p"),
    BnrCase("bnr_p16to16_640tiles", 5, 128, 256, 16, 16, density=0.25, tune=_CAP, kernel="halo_p", loops=True),
    BnrCase("bnr_p32to32_640tiles", 5, 128, 256, 32, 32, density=0.25, tune=_CAP, kernel="halo_p", loops=True),
    BnrCase("bnr_pool_p16to16_all", 1, 16, 64, 16, 16, pool_c0=16, kernel="halo_p"),
    BnrCase("bnr_pool_p32to32_all_640tiles", 5, 128, 256, 32, 32, pool_c0=32, density=0.25, tune=_CAP, kernel="halo_p", loops=True),
]
BNR_BY_NAME = {c.name: c for c in BNR_CASES}


@functools.lru_cache(maxsize=2)
def bnr_reference(c):
    """Inputs (fp32 CPU, NCHW) and fp64 expectations of one BNR case: dz (complete gradient), m, stored, s1 = sum dz m, s2 = sum dz m y."""
    g = _gen(c.name)
    r = {"x0": ternary((c.N, c.C0, c.H, c.W), g, c.density), "w": ternary((c.C0, c.Cout, 3, 3), g, c.density)}
    acc = F.conv_transpose2d(r["x0"].double(), r["w"].double(), padding=1)
    r["acc"] = acc
    if c.pool_c0:
        dz = F.avg_pool2d(acc[:, :c.pool_c0], 2) * 4
        r["prev_skip"] = ints((c.N, c.Cout - c.pool_c0, c.H, c.W), g, -8, 8) if c.skip_accumulate else None
        r["skip"] = acc[:, c.pool_c0:] + (r["prev_skip"].double() if c.skip_accumulate else 0)
    else:
        dz = acc
    r["prev"] = ints(tuple(dz.shape), g, -8, 8) if c.accumulate else None
    if c.accumulate:
        dz = dz + r["prev"].double()
    r["y"], r["scale"], r["shift"], r["out"], m = mask_inputs(g, tuple(dz.shape), c.from_out)
    r["dz"], r["m"] = dz, m
    r["stored"] = dz * m if c.bnr_mask else dz
    r["s1"] = (dz * m).sum(dim=(0, 2, 3))
    r["s2"] = (dz * m * r["y"].double()).sum(dim=(0, 2, 3))
    r["sabs"] = (dz * m * r["y"].double()).abs().sum(dim=(0, 2, 3))
    return r


def check_bnr_range(c, r):
    for k in ("acc", "dz", "skip"):
        if k in r and r[k].numel():
            assert float(r[k].abs().max()) <= 256, (c.name, "max |%s|" % k, float(r[k].abs().max()))
    assert float(r["sabs"].max()) < EXACT, (c.name, "sum |dz m y|", float(r["sabs"].max()))
    check_mask_variety(c.name, r["y"], r["scale"], r["shift"])
    if c.from_out:   # `out` disagrees with what y would give: the test tells the two mask sources apart
        my = (r["y"].double() * _v(r["scale"]) + _v(r["shift"]) > 0).double()
        assert float((my != r["m"]).double().mean()) > 0.2
        assert not torch.equal((r["dz"] * my).sum(dim=(0, 2, 3)), r["s1"])


def check_bnr_dispatch_and_loops(c):
    out = {}
    for dt in DTYPES:
        k = c.launch(dt)
        assert k[0] == c.want(dt), (c.name, dt, k)
        rows = c.grid_rows(dt)
        if k[0] == "halo_p" and c.loops:
            ntiles = c.N * c.H * c.W // 256
            most, fewest = E.tiles_per_workgroup(ntiles, rows)
            assert rows < ntiles and ntiles % rows and most > fewest >= 1, (c.name, dt, ntiles, rows)
            out[dt] = (ntiles, rows, most, fewest)
        if k[0].startswith("hg_"):
            bn = E.hg_shape(c.H, c.W, c.Cout)[2]
            assert not c.pool_c0 or c.pool_c0 % bn == 0, (c.name, "pool_c0 is a whole number of column blocks")
    return out


# ------------------------------------------------------------------------------------------------ b. bn_backward
def dyadic_bits(t):
    """Smallest q with t * 2^q integral everywhere, and max |t| * 2^q: t is exact in fp32 when the latter is below 2^24."""
    t = t.double().flatten()
    for q in range(0, 60):
        s = t * float(2 ** q)
        if bool((s == s.round()).all()):
            return q, float(s.abs().max())
    raise AssertionError("not a dyadic rational with fewer than 60 fractional bits")


def assert_dyadic(what, t):
    q, top = dyadic_bits(t)
    assert top < EXACT, (what, "needs", q, "fractional bits and reaches", top)


def bn_params(g, Cc):
    """mean in halves, invstd a power of two, gamma a small integer: every coefficient of the backward is a dyadic rational"""
    mean = ints((Cc,), g, -1, 2) / 2
    invstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (Cc,), generator=g)]
    gamma = torch.tensor([-1.0, 1.0, 2.0])[torch.randint(0, 3, (Cc,), generator=g)]
    return mean, invstd, gamma


def bn_backward_reference(dz, y, mean, invstd, gamma, exact=True):
    """fp64 BatchNorm backward from the masked gradient dz [rows][C] and the pre-BN tensor y, written as the kernels factor it:
    dy = k1 dz + k2 y + k3.  exact: assert that every intermediate is a dyadic rational fp32 holds."""
    rows = dz.shape[0]
    dz, y, mean, invstd = dz.double(), y.double(), mean.double(), invstd.double()
    gamma = torch.ones_like(mean) if gamma is None else gamma.double()
    a1 = dz.sum(0)
    s2 = (dz * y).sum(0)
    a2 = (s2 - mean * a1) * invstd
    gi = gamma * invstd
    m1, m2 = a1 / rows, a2 / rows
    k1, k2, k3 = gi, -gi * m2 * invstd, gi * (m2 * invstd * mean - m1)
    inner = k2 * y + k3
    dy = k1 * dz + inner
    assert float((dz * y).abs().sum(0).max()) < EXACT and float(dz.abs().sum(0).max()) < EXACT
    if exact:
        for what, t in (("a1", a1), ("a2", a2), ("m1", m1), ("m2", m2), ("k1", k1), ("k2", k2), ("k3", k3), ("k2 y + k3", inner), ("dy", dy)):
            assert_dyadic(what, t)
    return {"dgamma": a2, "dbeta": a1, "coef": torch.stack([k1, k2, k3]), "dy": dy}


@dataclass(frozen=True)
class BnCase:
    name: str
    C: int
    rows: int = 1024
    mask: str = "mscale"         # out | mscale | none | premasked
    accumulate_param: bool = False
    dres: str = ""               # "" | "write" | "accumulate"
    want_dy: bool = True
    pre_nblk: int = 0


BN_CASES = [
    BnCase("bn_mask_out_c64", 64, mask="out"),
    BnCase("bn_mask_mscale_c16", 16),
    BnCase("bn_no_relu_c512", 512, mask="none"),
    BnCase("bn_accumulate_param_c64", 64, accumulate_param=True),
    BnCase("bn_dres_write_c64", 64, mask="out", dres="write"),
    BnCase("bn_dres_accumulate_c16", 16, mask="out", dres="accumulate"),
    BnCase("bn_coefficients_only_c16", 16, want_dy=False),
    BnCase("bn_pre_nblk1_c64", 64, pre_nblk=1),
    BnCase("bn_pre_nblk9_c512", 512, mask="out", pre_nblk=9),
    BnCase("bn_pre_nblk640_c64", 64, pre_nblk=640),          # above the 256 threads of bn_bwd_finalize_kernel: column_sums_f64 loops
    BnCase("bn_premasked_nblk9_c64", 64, mask="premasked", pre_nblk=9),
    BnCase("bn_premasked_nblk640_c16", 16, mask="premasked", pre_nblk=640, dres="write"),
    BnCase("bn_rows16384_c16", 16, rows=2 ** 14),
    BnCase("bn_rows16384_out_c64", 64, rows=2 ** 14, mask="out", dres="write"),
]


@functools.lru_cache(maxsize=2)
def bn_reference(c):
    """Inputs as [rows][C] fp32 and the fp64 expectation of one bn_backward case.  dout is the gradient the kernel is handed:
    already dz for a premasked case."""
    g = _gen(c.name)
    shape = (1, c.C, c.rows, 1)
    y, scale, shift, out, m = mask_inputs(g, shape, c.mask == "out")
    flat = lambda t: None if t is None else t.view(c.C, c.rows).t().contiguous()
    dfull = flat(ternary(shape, g, 0.5))
    m = torch.ones_like(flat(m)) if c.mask == "none" else flat(m)
    dz = dfull.double() * m
    mean, invstd, gamma = bn_params(g, c.C)
    r = bn_backward_reference(dz, flat(y), mean, invstd, gamma)
    r.update(y=flat(y), out=flat(out), scale=scale, shift=shift, mean=mean, invstd=invstd, gamma=gamma, dz=dz,
             dout=dz.float() if c.mask == "premasked" else dfull)
    if c.accumulate_param:
        r["prev_dgamma"], r["prev_dbeta"] = ints((c.C,), g, -64, 64) / 4, ints((c.C,), g, -64, 64)
        r["dgamma"], r["dbeta"] = r["dgamma"] + r["prev_dgamma"].double(), r["dbeta"] + r["prev_dbeta"].double()
        assert_dyadic("dgamma", r["dgamma"])
    if c.dres:
        r["prev_dres"] = ints((c.rows, c.C), g, -8, 8) if c.dres == "accumulate" else None
        r["dres"] = dz + (r["prev_dres"].double() if c.dres == "accumulate" else 0)
    if c.pre_nblk:
        r["partial"] = block_partials(dz, r["y"], c.pre_nblk)
    return r


def block_partials(dz, y, nblk):
    """[2][C][nblk]: sum dz and sum dz y over nblk contiguous row blocks (any split that adds up is a valid producer)."""
    dz, y = dz.double(), y.double()
    p1 = torch.stack([b.sum(0) for b in torch.tensor_split(dz, nblk)], 1)
    p2 = torch.stack([b.sum(0) for b in torch.tensor_split(dz * y, nblk)], 1)
    return torch.stack([p1, p2])


def round_once(t, dt):
    """the fp64 reference rounded once to the compute dtype"""
    return t.to(torch.float32 if dt == "f32" else torch.bfloat16).double()


# ------------------------------------------------------------------------------------------------ c. the chain the network runs
# (BNR case, how bn_backward gets its mask): the data gradient's partial and stored gradient go straight into bn_backward
CHAIN_CASES = [
    ("bnr_mask_accsrc_hg128to128", "premasked"),
    ("bnr_mask_hg64to64", "premasked"),
    ("bnr_hg128to128_16x8_nwork15", "mscale"),
    ("bnr_out_acc_hg64to64", "out"),
    ("bnr_p16to16_small", "mscale"),          # 1 024 rows: a power of two, dy exact as well
    ("bnr_p32to32_640tiles", "mscale"),
]


@functools.lru_cache(maxsize=2)
def chain_reference(name):
    c = BNR_BY_NAME[name]
    r = bnr_reference(c)
    rows = c.N * r["dz"].shape[2] * r["dz"].shape[3]
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(rows, -1)
    g = _gen("chain" + name)
    mean, invstd, gamma = bn_params(g, c.Cy)
    pow2 = rows & (rows - 1) == 0
    b = bn_backward_reference(flat(r["dz"] * r["m"]), flat(r["y"]), mean, invstd, gamma, exact=pow2)
    for k in ("dgamma", "dbeta"):
        assert_dyadic(k, b[k])
    b.update(mean=mean, invstd=invstd, gamma=gamma, rows=rows, pow2=pow2)
    return b


# ------------------------------------------------------------------------------------------------ d. parity-class stride-2 data gradient
@dataclass(frozen=True)
class ParityCase:
    name: str
    N: int
    Ho: int            # extent of dY
    Wo: int
    Cf_in: int         # the FORWARD layer: Cf_in -> Cf_out, R x R, stride 2
    Cf_out: int
    R: int = 3
    accumulate: bool = False

    @property
    def pad(self):
        return 1 if self.R == 3 else 0

    def launch(self, dt):
        """profile name of the one gather-form launch (ncls = 4 rules out the 32-row tiles)"""
        if self.R == 3:
            bn = E._pick_bn(self.Cf_in)
            return "igemm", "conv_igemm_%s_%s" % (dt, {128: "128x128", 64: "128x64", 32: "256x32", 16: "256x16"}[bn])
        return E.conv_kernel(dt, self.N, self.Ho, self.Wo, self.Ho, self.Wo, self.Cf_out, 0, self.Cf_in, 1, 1, 1, 0)

    def class_kpad(self, dt):
        kstep = 32 if dt == "f32" else 64
        return [_rup(((2 if cls >> 1 else 1) * (2 if cls & 1 else 1)) * self.Cf_out, kstep) for cls in range(4)]


PARITY_CASES = [
    ParityCase("par_64to128_35px", 1, 5, 7, 64, 128),                  # 35 pixels per class: below one row tile, no multiple of 32
    ParityCase("par_128to256_720px", 3, 12, 20, 128, 256),             # 720 = 5 row tiles of 128 and a remainder, across images
    ParityCase("par_64to24_ragged_k", 1, 5, 7, 64, 24),                # K = 24, 48, 48, 96: a different zero-padded tail per class
    ParityCase("par_16to64_256row_tiles", 2, 12, 20, 16, 64),          # 480 pixels on 256-row tiles
    ParityCase("par_64to128_accumulate", 1, 5, 7, 64, 128, accumulate=True),
    ParityCase("par_1x1_64to128_accumulate", 3, 5, 7, 64, 128, R=1, accumulate=True),
    ParityCase("par_1x1_64to128_write", 3, 5, 7, 64, 128, R=1),
]


@functools.lru_cache(maxsize=2)
def parity_reference(c):
    g = _gen(c.name)
    dy = ternary((c.N, c.Cf_out, c.Ho, c.Wo), g, 0.5)
    w = ternary((c.Cf_out, c.Cf_in, c.R, c.R), g, 0.5)
    xshape = (c.N, c.Cf_in, 2 * c.Ho, 2 * c.Wo)
    x = torch.zeros(xshape, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), stride=2, padding=c.pad).backward(dy.double())
    prev = ints(xshape, g, -8, 8)
    dx = x.grad + (prev.double() if c.accumulate else 0)
    touched = torch.zeros(xshape, dtype=torch.bool)
    if c.R == 1:
        touched[:, :, ::2, ::2] = True     # a 1x1 stride-2 layer reaches the (even, even) pixels only
    else:
        touched[:] = True
    return {"dy": dy, "w": w, "prev": prev, "grad": x.grad, "dx": dx, "touched": touched}


def check_parity_case(c, r):
    assert float(r["grad"].abs().max()) <= 256 and float(r["dx"].abs().max()) <= 256, c.name
    assert tuple(r["grad"].shape[2:]) == (2 * c.Ho, 2 * c.Wo)
    if c.R == 1:
        assert float(r["grad"][~r["touched"]].abs().max()) == 0.0
    for dt in DTYPES:
        fam, name = c.launch(dt)
        assert fam == "igemm", (c.name, dt, fam)
    kp = [c.class_kpad(dt) for dt in DTYPES]
    if c.name == "par_64to24_ragged_k":
        assert all(len(set(k)) >= 2 for k in kp) and all(any(kk > t * c.Cf_out for kk, t in zip(k, (1, 2, 2, 4))) for k in kp)


# ------------------------------------------------------------------------------------------------ e. pack_weights_all
def rows_pad(c):
    return _rup(c, E._pick_bn(c))


def pack_table(dt):
    """One table for one launch: (descriptors as dicts of flair_pack_desc_t fields + name / branch, floats of params, arena bytes).
    branch: the part of pack_weights_all_kernel the descriptor runs in this dtype."""
    kstep, es = (32, 4) if dt == "f32" else (64, 2)
    bf = dt == "bf16"
    spec = [
        # name, Cout, Cin, R, Cin_p, tf, subset (r0, rstep, Rc, s0, sstep, Sc)
        ("fwd3x3_64to32", 32, 64, 3, 64, 0, None),
        ("fwd3x3_12to16_padded_cin", 16, 12, 3, 16, 0, None),
        ("fwd7x7_stem_5of8", 64, 5, 7, 8, 0, None),
        ("fwd1x1_64to128", 128, 64, 1, 64, 0, None),
        ("fwd3x3_16to13_rows16", 13, 16, 3, 16, 0, None),
        ("fwd3x3_16to16_tap_subset", 16, 16, 3, 16, 0, (0, 2, 2, 1, 2, 1)),
        ("tr3x3_32to64", 64, 32, 3, 64, 1, None),
        ("tr3x3_16to13", 13, 16, 3, 16, 1, None),
        ("tr3x3_48to64", 64, 48, 3, 64, 1, None),
        ("tr1x1_64to128", 128, 64, 1, 128, 1, None),
        ("tr5x5_8to16", 16, 8, 5, 16, 1, None),
    ] + [("tr3x3_64to128_class%d" % cls, 128, 64, 3, 128, 1,
          ((0 if cls >> 1 else 1), 2, (2 if cls >> 1 else 1), (0 if cls & 1 else 1), 2, (2 if cls & 1 else 1))) for cls in range(4)]
    descs, w_off, dst_off = [], 0, 256
    for name, Cout, Cin, R, Cin_p, tf, sub in spec:
        taps = sub[2] * sub[5] if sub else R * R
        d = dict(name=name, w_off=w_off, dst_off=dst_off, Cout=Cout, Cin=Cin, R=R, S=R, Cin_p=Cin_p, rows_pad=rows_pad(Cin if tf else Cout),
                 Kpad=_rup(taps * Cin_p, kstep), tf=tf, r0=0, rstep=0, Rc=0, s0=0, sstep=0, Sc=0)
        if sub:
            d.update(r0=sub[0], rstep=sub[1], Rc=sub[2], s0=sub[3], sstep=sub[4], Sc=sub[5])
        if not tf:
            d["branch"] = "fwd4" if (bf and R == 3 and not sub and Cin % 4 == 0) else "fwd"
        elif R * R > 9:
            d["branch"] = "large"
        else:
            d["branch"] = "tr_fast" if (bf and R == 3 and Cin % 32 == 0 and Cout % 32 == 0) else "tr"
        descs.append(d)
        w_off += _rup(Cout * Cin * R * R, 4)                      # 16-byte aligned masters, as in the flat parameter buffer
        dst_off += _rup(d["rows_pad"] * d["Kpad"] * es, 256) + 256   # a guard gap after every pack
    return descs, w_off, dst_off


def pack_params(nfloats):
    g = _gen("pack_params")
    # values bf16 holds exactly (so that both dtypes share one expectation) but not all integers: k / 4, |k| <= 12
    return ints((nfloats,), g, -12, 12) / 4


def pack_expected(d, params):
    """The layout formula above pack_weight_kernel, restated: fp32 [rows_pad][Kpad], zeros outside the real region."""
    w = params[d["w_off"]:d["w_off"] + d["Cout"] * d["Cin"] * d["R"] * d["S"]].numpy().reshape(d["Cout"], d["Cin"], d["R"], d["S"])
    dst = np.zeros((d["rows_pad"], d["Kpad"]), dtype=np.float32)
    if d["Rc"]:
        taps = [(d["r0"] + ri * d["rstep"], d["s0"] + si * d["sstep"]) for ri in range(d["Rc"]) for si in range(d["Sc"])]
    else:
        taps = [(r, s) for r in range(d["R"]) for s in range(d["S"])]
    for tp, (r, s) in enumerate(taps):
        col = tp * d["Cin_p"]
        if d["tf"]:   # dst[c][tap][k] = w[k][c][R-1-r][S-1-s]
            dst[:d["Cin"], col:col + d["Cout"]] = w[:, :, d["R"] - 1 - r, d["S"] - 1 - s].T
        else:         # dst[k][tap][c] = w[k][c][r][s]
            dst[:d["Cout"], col:col + d["Cin"]] = w[:, :, r, s]
    return dst


def check_pack_table():
    for dt in DTYPES:
        descs, nfl, nby = pack_table(dt)
        assert 12 <= len(descs) <= 64
        assert len({d["name"] for d in descs}) == len(descs)
        want = {"fwd", "tr", "large"} | ({"fwd4", "tr_fast"} if dt == "bf16" else set())
        assert {d["branch"] for d in descs} == want, dt
        for d in descs:
            assert d["w_off"] % 4 == 0 and d["dst_off"] % 256 == 0
            real_rows, real_cols = (d["Cin"], d["Cout"]) if d["tf"] else (d["Cout"], d["Cin"])
            taps = d["Rc"] * d["Sc"] if d["Rc"] else d["R"] * d["S"]
            assert d["rows_pad"] >= real_rows and d["Cin_p"] >= real_cols and d["Kpad"] >= taps * d["Cin_p"]
        # every kind of padding occurs: rows, channels inside a tap, the K tail
        assert any(d["rows_pad"] > (d["Cin"] if d["tf"] else d["Cout"]) for d in descs)
        assert any(d["Cin_p"] > (d["Cout"] if d["tf"] else d["Cin"]) for d in descs)
        assert any(d["Kpad"] > (d["Rc"] * d["Sc"] if d["Rc"] else d["R"] * d["S"]) * d["Cin_p"] for d in descs)
        p = pack_params(nfl)
        assert torch.equal(p.to(torch.bfloat16).float(), p)
        # the four class packs together hold each of the nine taps exactly once
        cls = [d for d in descs if "_class" in d["name"]]
        taps = sorted((d["r0"] + ri * d["rstep"], d["s0"] + si * d["sstep"]) for d in cls for ri in range(d["Rc"]) for si in range(d["Sc"]))
        assert taps == [(r, s) for r in range(3) for s in range(3)]


# ------------------------------------------------------------------------------------------------ f / g. pooling and elementwise shapes
POOL_SHAPE = (2, 12, 34)                       # N, H, W: with 64 channels a row has more than 256 chunks and no multiple of 256 (the
                                               # workgroup strides over it with a ragged last pass); with 16 channels fewer (idle threads)
POOL_CHANNELS = (64, 16)
UPCAT_CASES = [(2, 6, 10, 32, 64), (2, 6, 10, 64, 0), (4, 128, 256, 32, 64)]   # N, H, W, C0, C1; the last: past 4 096 workgroups
EW_BLOCK_CAP = 4096
COLSUM_CASE = (E.BN_BLOCK_CAP * 256 + 77, 16, 13)    # rows past bn_bwd_blocks' cap with a ragged tail, ld, C


def check_elementwise_shapes():
    N, H, W = POOL_SHAPE
    for Cc in POOL_CHANNELS:
        for ch in (4, 8):
            assert Cc % ch == 0 and 256 % (Cc // ch) == 0 and (W * (Cc // ch)) % 256
    assert all(W * (64 // ch) > 256 for ch in (4, 8)) and all(W * (16 // ch) < 256 for ch in (4, 8))
    assert H % 2 == 0 and W % 2 == 0
    N, H, W, C0, C1 = UPCAT_CASES[-1]
    for ch in (4, 8):
        assert N * (H // 2) * (W // 2) * (C0 // ch) + N * H * W * (C1 // ch) > EW_BLOCK_CAP * 256
    rows, ld, Cc = COLSUM_CASE
    assert rows > E.BN_BLOCK_CAP * 256 and rows % 256 and Cc < ld and rows < EXACT


# ------------------------------------------------------------------------------------------------ h. stem weight gradient, fused apply
STEM_CASES = [(2, 16, 32), (3, 24, 48)]         # N and the OUTPUT extent of the 8 -> 64, 7x7 / stride-2 / pad-3 stem: 8 and 27 tiles of 8x16


@functools.lru_cache(maxsize=2)
def stem_reference(shape):
    N, Ho, Wo = shape
    g = _gen("stem%dx%dx%d" % shape)
    x = ternary((N, 8, 2 * Ho, 2 * Wo), g, 0.5)
    x[:, 5:] = 0
    dout = ternary((N, 64, Ho, Wo), g, 0.5)
    y, scale, shift, _, m = mask_inputs(g, (N, 64, Ho, Wo), False)
    k1, k2, k3 = ints((64,), g, 1, 2), ints((64,), g, 0, 1), ints((64,), g, -1, 1)
    staged = _v(k1) * dout.double() * m + _v(k2) * y.double() + _v(k3)
    assert float(staged.abs().max()) <= 256
    dw = torch.nn.grad.conv2d_weight(x[:, :5].double(), (64, 5, 7, 7), staged, stride=2, padding=3)
    terms = (staged.abs().amax() * N * Ho * Wo)
    assert float(terms) < EXACT
    return {"x": x, "dout": dout, "y": y, "scale": scale, "shift": shift, "coef": torch.stack([k1, k2, k3]), "staged": staged, "dw": dw}


def check_stem_dispatch(shape):
    N, Ho, Wo = shape
    k = E.wgrad_kernel("bf16", N, 2 * Ho, 2 * Wo, Ho, Wo, 8, 0, 64, 7, 2, 3)
    assert k[0] == "stem", k
    return k
