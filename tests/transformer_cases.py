"""Case tables, input builders and fp64 references of the operator tests of the SegFormer / UperNet-Swin kernels
(tests/test_gpu_transformer_ops.py runs them on the GPU, tests/test_transformer_ops_cases_cpu.py checks their preconditions on
the references alone).  A plain module, not a conftest.

The references are restatements of the published algorithms (transformers' modeling_swin.py / modeling_segformer.py, torch.nn)
in plain torch fp64; the CPU test pins each against the installed library to 1e-12.  A bf16 reference takes the bf16-rounded
inputs and rounds to bf16 exactly where the kernel does; each such point is named in the reference's docstring.

The launch arithmetic of the kernels (query blocks of the attentions, the elementwise grid cap, the depth-wise grid cap, the
LayerNorm group sizes) is restated here so that the CPU test can assert that a case written for a loop really loops."""
import math

import torch
import torch.nn.functional as F

DTYPES = ("f32", "bf16")
TUNE_DEFAULTS = {"FLAIR_SF_ATT2": 1, "FLAIR_SF_FFN": 1, "FLAIR_SF_HEAD": 2, "FLAIR_SF_DW_L": 0}
TOL = {"f32": 2e-4, "bf16": 3e-2}   # the standing operator tolerances (test_gpu_ops.py): no measured bound may exceed them


def bf16r(x):
    """fp64 -> the nearest bf16 (through fp32, as the kernels round), back in fp64"""
    return x.float().to(torch.bfloat16).double()


def rnd(x, dt):
    return bf16r(x) if dt == "bf16" else x.float().double()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randint(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def nonzero_int(g, m, *shape):
    """integers in [-m, m] without 0"""
    v = torch.randint(1, m + 1, shape, generator=g).double()
    return v * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def ulp(x, mant):
    """unit in the last place of |x| for a format with `mant` stored significand bits (23: fp32, 7: bf16)"""
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - mant)


# ------------------------------------------------------------------------------------------------ launch arithmetic, restated
def att_qblocks(two_tile, B, heads, N):
    """attention_launch / attention2_launch (segformer_ops.hip): query blocks a workgroup walks"""
    step, cap = (128, 4) if two_tile else (64, 8)
    qb = 1
    while qb < cap and -(-N // (step * qb * 2)) * heads * B >= 512:
        qb *= 2
    return qb


def att_walk(two_tile, B, heads, N):
    """(qblocks, grid.x, does some workgroup break early, does a walked block have a ragged tail)"""
    step = 128 if two_tile else 64
    qb = att_qblocks(two_tile, B, heads, N)
    gx = -(-N // (step * qb))
    last0 = (gx - 1) * qb * step
    blocks_live = -(-(N - last0) // step)
    return qb, gx, blocks_live < qb, N % 16 != 0 or N % step != 0


def ew_blocks(total):
    return max(1, min((total + 255) // 256, 4096))


def ew_trips(total):
    """(trips of the busiest thread, chunks in the last trip) of a grid-stride elementwise kernel"""
    per = ew_blocks(total) * 256
    return -(-total // per), total - (-(-total // per) - 1) * per


def dw_launch(dt, B, H, W, C, lmax=0):
    """sf_dwconv3x3_gelu: (L, channel groups per workgroup, grid.x, grid.y, trips of the busiest pixel lane)"""
    ng = C // 4
    cg = 1
    while cg * 2 <= 256 and ng % (cg * 2) == 0:
        cg *= 2
    L = 16 if W % 16 == 0 else 8 if W % 8 == 0 else 4 if W % 4 == 0 else 2 if W % 2 == 0 else 1
    if lmax <= 0:
        lmax = 16 if dt == "f32" else 4
    while L > lmax and L > 1:
        L >>= 1
    items = B * H * (W // L)
    npl = 256 // cg
    gx = max(1, min(-(-items // npl), 8192))
    return L, cg, gx, ng // cg, -(-items // (gx * npl))


def sf_ln_group(dt, C):
    """layernorm_t: lanes per row, or None where the launcher refuses (more than two chunks per lane)"""
    nch = C // (4 if dt == "f32" else 8)
    G = 1
    while G < nch and G < 64:
        G <<= 1
    return None if nch > 2 * G else G


def swin_ln_group(dt, C):
    """ln_launch: (lanes per row, chunks of the busiest lane), or None where it refuses"""
    nch = C // (4 if dt == "f32" else 8)
    if nch > 64 * 6:
        return None
    G = 16 if nch <= 96 else 32 if nch <= 192 else 64
    return G, -(-nch // G)


# ---------------------------------------------------------------------------------------------------------------- references
def layernorm_ref(x, g, b, eps):
    """nn.LayerNorm over the last axis: biased variance of the centred values, eps inside the root"""
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * g + b


def patch_merge_ref(x, g, b, eps):
    """SwinPatchMerging up to its reduction: cat [x(0::2, 0::2) | x(1::2, 0::2) | x(0::2, 1::2) | x(1::2, 1::2)], LayerNorm(4C)"""
    cat = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
    return layernorm_ref(cat, g, b, eps)


def window_slots(H, W, shift):
    """Addressing of the shifted-window attention: for the grid padded to multiples of 7 and rolled by -shift,
    tok [nwin][49] = flat token index (y * W + x) of every window slot or -1 for a pad token, lab [nwin][49] = the region label
    of SwinLayer.get_attn_mask (all 0 without shift)."""
    Hp, Wp = -(-H // 7) * 7, -(-W // 7) * 7
    sy, sx = torch.meshgrid(torch.arange(Hp), torch.arange(Wp), indexing="ij")
    oy, ox = (sy + shift) % Hp, (sx + shift) % Wp          # torch.roll(x, -shift): position s holds the token of s + shift
    tok = torch.where((oy < H) & (ox < W), oy * W + ox, torch.full_like(oy, -1))
    if shift:
        lab = 3 * ((sy >= Hp - 7).long() + (sy >= Hp - shift).long()) + (sx >= Wp - 7).long() + (sx >= Wp - shift).long()
    else:
        lab = torch.zeros_like(sy)

    def part(t):
        return t.view(Hp // 7, 7, Wp // 7, 7).permute(0, 2, 1, 3).reshape(-1, 49)
    return part(tok), part(lab)


def rel_index():
    """SwinRelativePositionBias: index [49 queries][49 keys] into the [169][heads] table, (qy - ky + 6) * 13 + (qx - kx + 6)"""
    p = torch.arange(49)
    y, x = p // 7, p % 7
    return (y[:, None] - y[None, :] + 6) * 13 + (x[:, None] - x[None, :] + 6)


def window_attention_ref(qkv, qkv_bias, table, heads, shift, round_p=False):
    """qkv [B][H][W][3C] fp64 (biases included) -> [B][H][W][C].  Pad tokens are zeros after the LayerNorm, so their q, k, v are
    the projection biases; they take part as keys and values and are cropped as queries.  Scores q.k * 32^-0.5 + table[rel] +
    mask (-100 between different regions of a shifted block, not -inf).
    round_p (the bf16 kernel): P = exp(s - max) is rounded to bf16 before the second product while the softmax denominator is
    the sum of the unrounded values (swin_ops.hip, swin_attention_kernel: `sum += acc` before the `f32_to_bf16(acc...)` pack)."""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    tok, lab = window_slots(H, W, shift)
    flat = torch.cat([qkv.reshape(B, H * W, C3), qkv_bias.view(1, 1, C3).expand(B, 1, C3)], 1)   # row H * W: the pad token
    idx = torch.where(tok >= 0, tok, torch.full_like(tok, H * W))
    win = flat[:, idx]                                            # [B][nwin][49][3C]
    nw = idx.shape[0]
    q, k, v = (win[..., i * C:(i + 1) * C].reshape(B, nw, 49, heads, 32).permute(0, 1, 3, 2, 4) for i in range(3))
    s = q @ k.transpose(-1, -2) * 32 ** -0.5
    s = s + table[rel_index()].permute(2, 0, 1)[None, None]
    s = s + torch.where(lab[:, :, None] != lab[:, None, :], -100.0, 0.0)[None, :, None]
    p = torch.exp(s - s.amax(-1, keepdim=True))
    den = p.sum(-1, keepdim=True)
    o = ((bf16r(p) if round_p else p) @ v) / den                  # [B][nw][heads][49][32]
    o = o.permute(0, 1, 3, 2, 4).reshape(B, nw * 49, C)
    out = torch.zeros(B, H * W + 1, C, dtype=torch.float64)
    out[:, idx.reshape(-1)] = o                                   # pad slots all land in the spare row
    return out[:, :H * W].reshape(B, H, W, C)


def sf_attention_ref(q, k, v, round_p=False):
    """softmax(Q K^T / 8) V per head of 64 channels; q [B][N][hidden], k, v [B][Nk][hidden].
    round_p (bf16 kernels): P = exp(s - max) rounded to bf16 before the second product, the denominator from the unrounded
    values (segformer_ops.hip, attention_kernel: `sum += acc` before the pack; attention2_kernel: `ps += acc` likewise)."""
    B, N, hid = q.shape
    h = hid // 64
    qh, kh, vh = (t.reshape(B, -1, h, 64).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / 8
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = ((bf16r(p) if round_p else p) @ vh) / p.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(B, N, hid)


def gelu_ref(v):
    return 0.5 * v * (1 + torch.erf(v / math.sqrt(2.0)))


def dwconv_gelu_ref(x, w, b):
    """x [B][H][W][C], w [C][3][3], b [C] -> (pre-activation, erf-GELU of it), NHWC"""
    pre = F.conv2d(x.permute(0, 3, 1, 2), w[:, None], b, padding=1, groups=x.shape[-1]).permute(0, 2, 3, 1)
    return pre, gelu_ref(pre)


def mix_ffn_ref(x, p, eps, faithful=False, ln2=None):
    """The Mix-FFN of a SegformerLayer with the norm and the residual around it:
    out = x + fc2(gelu(dwconv3x3(fc1(LayerNorm(x))))), x [B][H][W][C]; p = dict(ln_g, ln_b, w1 [4C][C], b1, dw_w [4C][3][3], dw_b,
    w2 [C][4C], b2).  ln2 = (g, b): also LayerNorm(out).
    faithful (ffn_fused_kernel, segformer_ops.hip): bf16 roundings of the LayerNorm output (`f_to_chunk` in the in-place norm), of
    fc1's output + bias (`pk` before the store to h1; the conv pads THAT with zeros), of the GELU output (`pk` before the store
    to a2), of the block result (`pk` before the store to out) and of LayerNorm(out) computed FROM the rounded result (`xo`)."""
    r = bf16r if faithful else (lambda t: t)
    xn = r(layernorm_ref(x, p["ln_g"], p["ln_b"], eps))
    h1 = r(xn @ p["w1"].T + p["b1"])
    a2 = r(dwconv_gelu_ref(h1, p["dw_w"], p["dw_b"])[1])
    out = r(a2 @ p["w2"].T + p["b2"] + x)
    if ln2 is None:
        return out, None
    return out, r(layernorm_ref(out, ln2[0], ln2[1], eps))


def interp_matrix(n_in, n_out):
    """1-D weights [n_out][n_in] of F.interpolate(mode='bilinear', align_corners=False): src = max(0, (dst + 0.5) n_in / n_out - 0.5)"""
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        s = max(0.0, (o + 0.5) * n_in / n_out - 0.5)
        i0 = min(int(s), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        m[o, i0] += 1 - (s - i0)
        m[o, i1] += s - i0
    return m


def bilinear_ref(x, H, W):
    """x [B][h][w][C] -> [B][H][W][C]"""
    t = torch.einsum("Hh,bhwc->bHwc", interp_matrix(x.shape[1], H), x)
    return torch.einsum("Ww,bHwc->bHWc", interp_matrix(x.shape[2], W), t)


def avgpool_ref(x, S):
    """nn.AdaptiveAvgPool2d(S) on NHWC: bin i spans [floor(i n / S), ceil((i + 1) n / S))"""
    B, h, w, C = x.shape
    out = torch.empty(B, S, S, C, dtype=torch.float64)
    for i in range(S):
        for j in range(S):
            out[:, i, j] = x[:, i * h // S:-(-(i + 1) * h // S), j * w // S:-(-(j + 1) * w // S)].mean((1, 2))
    return out


def pool_bins(n, S):
    return [-(-(i + 1) * n // S) - i * n // S for i in range(S)]


def head_core_ref(f0, w0, g1, g2, g3, scale, shift2, wc, bc, round_z=False):
    """The decode head after the per-stage products (head_fused_kernel / upsample_sum_bn_relu_kernel):
    z = relu(scale * (W0 f0 + up(g1) + up(g2) + up(g3)) + shift2), logits = Wc z + bc; f0 [B][H][W][64], g_i [B][H >> i][W >> i][D].
    Returns (z NHWC, logits NCHW).  round_z: z rounded to bf16 before the classifier product (`zp` in head_fused_kernel)."""
    B, H, W, _ = f0.shape
    acc = f0 @ w0.T
    for g in (g1, g2, g3):
        acc = acc + bilinear_ref(g, H, W)
    z = torch.relu(acc * scale + shift2)
    zz = bf16r(z) if round_z else z
    return z, (zz @ wc.T + bc).permute(0, 3, 1, 2)


def fuse_bias_ref(wf, b3, b2, b1, b0, scale, shift):
    return shift + scale * (wf @ torch.cat([b3, b2, b1, b0]))


def decode_head_ref(feats, proj_w, proj_b, fuse_w, bn_scale, bn_shift, cls_w, cls_b):
    """SegformerDecodeHead in eval mode, restructured as the kernels compute it: everything before the BatchNorm is linear and a
    per-channel resize commutes with a per-pixel channel mix, so fuse(cat_i up(P_i f_i + b_i)) = sum_i up((F_i P_i) f_i) + F bcat
    with F_i the column block of the fuse weight that meets stage i (the concatenation is stage 3 first).
    feats: 4 NHWC stage outputs; proj_w[i] [D][C_i]; fuse_w [D][4D]; bn_* the folded BatchNorm."""
    D = fuse_w.shape[0]
    fw = [fuse_w[:, (3 - i) * D:(4 - i) * D] @ proj_w[i] for i in range(4)]
    shift2 = fuse_bias_ref(fuse_w, proj_b[3], proj_b[2], proj_b[1], proj_b[0], bn_scale, bn_shift)
    g = [feats[i] @ fw[i].T for i in range(1, 4)]
    return head_core_ref(feats[0], fw[0], g[0], g[1], g[2], bn_scale, shift2, cls_w, cls_b)[1]


def wint_ref():
    """sf_head_wint in closed form: [128 pixels of a 16 x 8 tile][96 source pixels]; source s is (stage, row, column) of the
    stage's patch (6 x 10, 4 x 6, 3 x 4) that starts one source pixel before the tile's first; the weight is the product of the
    two 1-D weights of an unclamped x 2^stage resize."""
    m = torch.zeros(128, 96, dtype=torch.float64)

    def w1(o, idx, st):
        sc = (o + 0.5) / (1 << st) - 0.5
        fl = math.floor(sc)
        i0 = fl + 1
        return 1 - (sc - fl) if idx == i0 else (sc - fl) if idx == i0 + 1 else 0.0
    for px in range(128):
        for s in range(96):
            st, r = (1, s) if s < 60 else (2, s - 60) if s < 84 else (3, s - 84)
            cols = {1: 10, 2: 6, 3: 4}[st]
            m[px, s] = w1(px // 16, r // cols, st) * w1(px % 16, r % cols, st)
    return m


# ---------------------------------------------------------------------------------------------------- attention as a gather
def _codes(n, bits, reps, width, amp):
    """[n][width]: +-amp by the bits of the index, each bit repeated over `reps` channels; the remaining channels zero"""
    i = torch.arange(n)
    c = torch.zeros(n, width, dtype=torch.float64)
    for b in range(bits):
        c[:, b * reps:(b + 1) * reps] = (((i >> b) & 1) * 2 - 1).double()[:, None] * amp
    return c


# (name, dtype, att2, B, heads, N, Nk, what the case is for)
SF_GATHER_CASES = [
    ("nk16_n16", "bf16", 1, 2, 1, 16, 16, "one key tile, one query tile"),
    ("nk144_n40", "bf16", 1, 2, 1, 40, 144, "a single 16-key tile in the second half of the online softmax; ragged tail"),
    ("nk256_n200_h8", "bf16", 1, 1, 8, 200, 256, "both halves full, 8 heads, ragged tail in the second workgroup"),
    ("one_tile_nk144_n40", "bf16", 0, 2, 1, 40, 144, "one-tile bf16 kernel, odd tile count (the `two` guard)"),
    ("one_tile_nk256_n200_h8", "bf16", 0, 1, 8, 200, 256, "one-tile bf16 kernel, all 16 key tiles"),
    ("one_tile_nk16_n16", "bf16", 0, 2, 1, 16, 16, "one-tile bf16 kernel, one key tile"),
    ("f32_nk16_n16", "f32", 1, 2, 1, 16, 16, "fp32 kernel"),
    ("f32_nk144_n40", "f32", 1, 2, 1, 40, 144, "fp32 kernel, ragged"),
    ("f32_nk256_n200_h8", "f32", 1, 1, 8, 200, 256, "fp32 kernel, 8 heads"),
    ("walk2_two_tile", "bf16", 1, 8, 8, 2048 + 40, 64, "qblocks = 2 in the two-tile kernel: prefetch, break, clamp inside a walked block"),
    ("walk4_two_tile", "bf16", 1, 8, 8, 8192, 64, "qblocks = 4 in the two-tile kernel"),
    ("walk2_one_tile", "bf16", 0, 8, 8, 1024 + 24, 64, "qblocks = 2 in the one-tile bf16 kernel"),
    ("walk2_f32", "f32", 1, 8, 8, 1024 + 24, 64, "qblocks = 2 in the fp32 kernel"),
]
SF_WALKED = {"walk2_two_tile": 2, "walk4_two_tile": 4, "walk2_one_tile": 2, "walk2_f32": 2}


def sf_gather_inputs(case):
    """q [B][N][hidden], kv [B][Nk][2 hidden] (k | v), expected out [B][N][hidden] — all fp64 holding bf16-exact integers.
    Key j of every head carries +-8 by the 8 bits of j, each over 8 channels; query i is 8 x the code of its target: the target's
    score is 64 * 64 / 8 = 512 and every other key's at most 64 * 48 / 8 = 384, 128 below."""
    name, dt, att2, B, heads, N, Nk, _ = case
    g = gen(sum(map(ord, name)))
    hid = 64 * heads
    code = _codes(256, 8, 8, 64, 8.0)
    tgt = torch.randint(0, Nk, (B, heads, N), generator=g)
    q = code[tgt].permute(0, 2, 1, 3).reshape(B, N, hid)          # a = 1 on codes of amplitude 8: q = +-8
    k = code[:Nk].view(1, Nk, 1, 64).expand(B, Nk, heads, 64).reshape(B, Nk, hid)
    v = nonzero_int(g, 255, B, Nk, heads, 64)
    want = torch.gather(v.permute(0, 2, 1, 3), 2, tgt[..., None].expand(B, heads, N, 64)).permute(0, 2, 1, 3).reshape(B, N, hid)
    return q, torch.cat([k, v.reshape(B, Nk, hid)], -1).contiguous(), want, tgt


# (name, B, H, W, heads, shift)
SWIN_GRIDS = [(2, 2), (4, 4), (7, 7), (8, 16), (14, 14)]
SWIN_GATHER_CASES = [(f"{h}x{w}_s{s}", 1, h, w, 3, s) for (h, w) in SWIN_GRIDS for s in (0, 3)] + [("8x16_s3_h24_b2", 2, 8, 16, 24, 3)]
SWIN_MASK_NAMES = ("4x4_s3", "7x7_s3", "14x14_s3")   # the grids where a window holds real tokens of more than one region
PAD_CODE = 63   # key code of the pad tokens: no slot has this index, so no query selects it


def swin_gather_inputs(case, decoys=False):
    """qkv [B][H][W][3C], qkv_bias [3C], expected out [B][H][W][C] (fp64 holding bf16-exact integers), and the two decoy counts.
    Key code: +-8 by the 6 bits of the token's slot in its window, each over 5 of the head's 32 channels (30 used); query = the
    code of its target, a real token of the same window AND region: target 64 * 30 * 32^-0.5 = 339.4, any other key at most
    64 * 20 * 32^-0.5 = 226.3, 113.1 below.  Pad tokens carry code 63 through qkv_bias.
    decoys (shift 3): in every window that straddles regions, one query gets a key of ANOTHER region raised through spare
    channel 30 to a raw advantage of 50 .. 56 over its target (the -100 mask must leave the target the winner, the decoy at
    e^-44 or less), a second through channel 31 to 150 .. 156 (the decoy must win: the mask is -100, not -inf)."""
    name, B, H, W, heads, shift = case
    g = gen(1000 + sum(map(ord, name)) + (7 if decoys else 0))
    C = 32 * heads
    tok, lab = window_slots(H, W, shift)
    code = _codes(64, 6, 5, 32, 8.0)
    q = torch.zeros(B, H * W, heads, 32, dtype=torch.float64)
    k = torch.zeros(B, H * W, heads, 32, dtype=torch.float64)
    v = nonzero_int(g, 255, B, H * W, heads, 32)
    want = torch.zeros(B, H * W, heads, 32, dtype=torch.float64)
    scale = 32 ** -0.5
    ndec = [0, 0]   # queries with a 50-advantage decoy, with a 150-advantage decoy
    for wi in range(tok.shape[0]):
        real = [j for j in range(49) if tok[wi, j] >= 0]
        for j in real:
            k[:, tok[wi, j]] = code[j]
        labels = sorted({int(lab[wi, j]) for j in real})
        picked = {}
        if decoys and len(labels) > 1:
            home = max(labels, key=lambda a: sum(int(lab[wi, j]) == a for j in real))
            inside = [j for j in real if int(lab[wi, j]) == home]
            outside = [j for j in real if int(lab[wi, j]) != home]
            d = outside[int(torch.randint(0, len(outside), (1,), generator=g))]
            for ch, adv, qj in ((30, 50.0, inside[0]), (31, 150.0, inside[-1])):
                if ch == 31 and len(inside) < 2:
                    continue
                picked[qj] = (ch, adv, d)
        for j in real:
            same = [t for t in real if lab[wi, t] == lab[wi, j]]
            t = torch.tensor(same)[torch.randint(0, len(same), (B, heads), generator=g)]       # [B][heads]
            q[:, tok[wi, j]] = code[t]
            win = t
            if j in picked:
                ch, adv, d = picked[j]
                t0 = same[0]
                q[:, tok[wi, j]] = code[t0]
                hd = bin(t0 ^ d).count("1")
                y = math.ceil((adv / scale + 640 * hd) / 32)       # raw score(d) - score(t0) = (32 y - 640 hd) * scale in [adv, adv + 5.7)
                q[:, tok[wi, j], :, ch] = 32.0
                k[:, tok[wi, d], :, ch] = float(y)
                win = torch.full((B, heads), d if adv > 100 else t0)
                ndec[adv > 100] += 1
            src = tok[wi][win]                                      # [B][heads] token indices
            want[:, tok[wi, j]] = v[torch.arange(B)[:, None], src, torch.arange(heads)[None, :]]
    bias = torch.zeros(3, heads, 32, dtype=torch.float64)
    bias[1] = code[PAD_CODE]
    bias[2] = randint(g, 1, 9, heads, 32)
    bias[0] = code[PAD_CODE]
    qkv = torch.cat([q.reshape(B, H, W, C), k.reshape(B, H, W, C), v.reshape(B, H, W, C)], -1).contiguous()
    return qkv, bias.reshape(-1), want.reshape(B, H, W, C), ndec


# ---------------------------------------------------------------------------------------------------------- fused decode head
# (H, W, D, labels): one tile where every source pixel clamps; interior + edge tiles; a non-square grid
HEAD_CASES = [(8, 16, 64, 1), (16, 32, 256, 13), (24, 16, 768, 19), (8, 16, 256, 32), (16, 32, 64, 19)]


def head_inputs(case, B=2):
    """Exact by construction.  The 2-D interpolation weights of the x2, x4, x8 resizes are a b / 4^(s+1) (odd a, b < 2^(s+1): 1-D
    denominators 4, 8, 16), so g1, g2 in multiples of 64 and g3 in multiples of 256 make every upsampled term an integer;
    f0, W0 ternary, scale 1, integer shift2 -> the accumulator is an integer; ternary Wc, integer bc.  z must be exact in bf16
    (an integer <= 256) and a full-weight g3 pixel alone is 256, so the other terms are kept non-positive where g3 is positive:
    g3 in {0, 256}, g1, g2 in {-64, 0}, shift2 in [-48, -32] against |W0 f0| <= 32: -208 <= acc + shift2 <= 256."""
    H, W, D, labels = case
    g = gen(H * 1000 + W * 10 + D + labels)
    d = dict(f0=randint(g, -1, 1, B, H, W, 64) * randint(g, 0, 1, B, H, W, 64), w0=randint(g, -1, 1, D, 64),
             g1=-64 * randint(g, 0, 1, B, H // 2, W // 2, D), g2=-64 * randint(g, 0, 1, B, H // 4, W // 4, D),
             g3=256 * randint(g, 0, 1, B, H // 8, W // 8, D), scale=torch.ones(D, dtype=torch.float64),
             shift2=randint(g, -48, -32, D), wc=randint(g, -1, 1, labels, D), bc=randint(g, -5, 5, labels))
    return d


def check_head_exact(d):
    acc = d["f0"] @ d["w0"].T
    assert float(acc.abs().max()) <= 32
    pre = acc
    for gi in (d["g1"], d["g2"], d["g3"]):
        pre = pre + bilinear_ref(gi, acc.shape[1], acc.shape[2])
    pre = pre + d["shift2"]
    assert torch.equal(pre, pre.round()) and float(pre.abs().max()) <= 256, float(pre.abs().max())
    z, logits = head_core_ref(**d)
    assert float(logits.abs().max()) < 2 ** 24 and float((z @ d["wc"].abs().T).max()) < 2 ** 24 and float((z > 0).double().mean()) > 0.2
    return z, logits


# ------------------------------------------------------------------------------------------------- depth-wise 3x3 + GELU cases
# (name, B, H, W, C, FLAIR_SF_DW_L (0 = default), what for)
DW_CASES = ([(f"w{w}_h{h}_c{c}", 2, h, w, c, 0, "default segment length") for (w, h, c) in
             [(16, 5, 4), (24, 2, 256), (12, 1, 1280), (6, 5, 256), (7, 2, 4), (16, 1, 256)]] +
            [(f"L{l}_w16_h5_c256", 1, 5, 16, 256, l, f"segment length pinned to {l}") for l in (1, 2, 4, 8, 16)] +
            [("cap_184x184_c256_L1", 1, 184, 184, 256, 1, "more than 8192 workgroups of work: the capped grid strides")])


def dw_inputs(case):
    name, B, H, W, C, _, _ = case
    g = gen(sum(map(ord, name)))
    return randint(g, -2, 2, B, H, W, C), randint(g, -2, 2, C, 3, 3), randint(g, -2, 2, C)


def gelu_bound(dt, pre, ref):
    """|kernel - fp64 erf-GELU| allowed when the pre-activation `pre` is exact.
    fp32 (0.5 v (1 + erff(v * 0.70710678f))): erff within 2 ulp of a value of magnitude <= 1 (2 * 2^-24 absolute), its argument
    rounded once (relative 2^-24, times erf'(a) a <= 0.48), the sum 1 + erf rounded once (2^-24): under 3.5 * 2^-24 absolute on
    (1 + erf), which the factor |v| / 2 carries to the result -> 2 |v| 2^-24 rounded up; then two multiplications, each half an
    ulp of the result, allowed 2 ulp.  (The absolute term is what matters in the negative tail, where 1 + erf cancels.)
    bf16 (h = erfc(|v| / sqrt 2) / 2 by Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7 on erfc so 0.75e-7 on h; v_rcp and v_exp at
    1 ulp each and five fused multiply-adds on values <= 0.5: 7 * 2^-24 = 4.2e-7 relative to h <= 0.5, 2.1e-7 absolute; the last
    product once more): under 4e-7 absolute on h, times |v|; then ONE rounding to bf16: half an ulp, allowed 1 ulp because
    an error of 4e-7 |v| on a value next to a rounding boundary moves the result to the neighbouring bf16."""
    if dt == "f32":
        return 2 * ulp(ref, 23) + 2 * pre.abs() * 2.0 ** -24
    return ulp(ref, 7) + 4e-7 * pre.abs()


# --------------------------------------------------------------------------------------------------- elementwise loop cases
def _loop(total):
    trips, last = ew_trips(total)
    return total > 1048576 and (total - 1048576) % 256 != 0 and trips == 2


# bf16 chunks = 8 elements.  name -> (shape parameters, chunk count)
EW_LOOP = {
    "swin_bilinear_add": dict(B=1, h=515, w=511, C=8, chunks=1 * 1030 * 1022 * 1),
    "sf_bilinear_nhwc": dict(B=1, h=515, w=511, C=8, ld=16, chunks=1 * 1030 * 1022 * 1),
    "swin_avgpool": dict(B=8, h=4, w=4, C=29128, S=6, chunks=8 * 36 * 3641),
    "sf_upsample_sum_bn_relu": dict(B=1, H=1040, W=1016, D=8, chunks=1040 * 1016),
    "sf_slice_cols": dict(rows=1048576 + 100, ld=16, col0=8, ncols=8, chunks=1048576 + 100),
}

# --------------------------------------------------------------------------------------------------------- LayerNorm cases
SF_LN_C = (64, 128, 320, 512)
SWIN_LN_C = (96, 192, 384, 768)
MERGE_C = (96, 384, 768)       # 4C = 384, 1536 (the widest merge of the network), 3072 (bf16 only: fp32 would need 12 chunks per lane)
MERGE_GRIDS = ((2, 2), (4, 6), (2, 8))
LN_KINDS = ("plain", "mean100", "tinyvar_eps1e-5", "tinyvar_eps1e-6")


def ln_rows(kind, rows, C, g):
    """(x, eps): rows with mean 100 and deviation 1 survive only if the variance is taken from centred values; rows whose
    variance is about 1e-6 make the output depend on eps by tens of percent"""
    x = torch.randn(rows, C, generator=g, dtype=torch.float64)
    if kind == "mean100":
        return 100 + x, 1e-5
    if kind.startswith("tinyvar"):
        return 0.25 + 1e-3 * x, (1e-5 if kind.endswith("1e-5") else 1e-6)
    return x, 1e-5


# ---------------------------------------------------------------------------------------------------------------- GEMM cases
# the gather-form GEMM as the transformer paths use it: (name, rows as (N, H, W), Cin, Cout, R, stride, pad)
GEMM_CASES = [("lin_16_96", (1, 4, 4), 96, 96, 1, 1, 0), ("lin_49_288", (1, 7, 7), 96, 288, 1, 1, 0),
              ("lin_130_192", (2, 5, 13), 96, 192, 1, 1, 0), ("lin_130_768", (2, 5, 13), 192, 768, 1, 1, 0),
              ("patch4", (2, 16, 24), 8, 96, 4, 4, 0), ("patch7", (2, 16, 24), 8, 64, 7, 4, 3), ("patch3", (2, 10, 14), 64, 128, 3, 2, 1),
              ("sr8", (2, 16, 16), 64, 64, 8, 8, 0), ("sr2", (1, 6, 10), 320, 320, 2, 2, 0)]


def gemm_inputs(case):
    name, (N, H, W), Cin, Cout, R, stride, pad = case
    g = gen(sum(map(ord, name)))
    x = randint(g, -1, 1, N, Cin, H, W)
    # the weights are thinned to about 40 per output so that |sum| stays within 256 (asserted on the reference)
    w = randint(g, -1, 1, Cout, Cin, R, R) * (torch.rand(Cout, Cin, R, R, generator=g) < min(1.0, 40.0 / (R * R * Cin))).double()
    b = randint(g, -3, 3, Cout)
    return x, w, b


# ------------------------------------------------------------------ the softmax denominator comes from the UNROUNDED P (bf16)
def denominator_inputs(Nk=256, N=40, heads=2):
    """q [1][N][hidden], kv [1][Nk][2 hidden] and the expected output BEFORE its final rounding.
    Every query is e_0 and key j >= 1 is -16 e_0: key 0 scores 0 (P = 1), every other key -16 / 8 = -2, P = exp(-2) = 0.135335,
    which lies 0.58 of a bf16 ulp above its lower neighbour: it rounds UP by 0.30 %, robustly (a tie is 0.08 ulp = 6e-4 relative
    away, the kernels' exp is good to 1e-6).  V is the same value c for every key of a channel, so
      numerator from rounded P, denominator from unrounded P (the kernels):  c (1 + 255 r(x)) / (1 + 255 x) = c (1 + 0.292 %)
      both from rounded P (or both unrounded):                               c exactly.
    c = +-(2 - j / 128) 2^e, j = 1 .. 6: just below a power of two, where half a bf16 ulp is 0.20 % of the value."""
    hid = 64 * heads
    q = torch.zeros(1, N, heads, 64, dtype=torch.float64)
    q[..., 0] = 1.0
    k = torch.zeros(1, Nk, heads, 64, dtype=torch.float64)
    k[:, 1:, :, 0] = -16.0
    ch = torch.arange(hid)
    c = (2 - ((ch % 6) + 1) / 128.0) * torch.exp2(((ch // 6) % 5 - 2).double()) * (1 - 2 * ((ch // 30) % 2)).double()
    v = c.view(1, 1, hid).expand(1, Nk, hid)
    x = torch.tensor(math.exp(-2.0), dtype=torch.float64)
    want = c * (1 + (Nk - 1) * bf16r(x)) / (1 + (Nk - 1) * x)
    return q.reshape(1, N, hid), torch.cat([k.reshape(1, Nk, hid), v], -1).contiguous(), want.view(1, 1, hid).expand(1, N, hid), c


def denominator_bound(ref):
    """half a bf16 ulp for the one rounding of the output, plus the fp32 arithmetic in front of it: two sums of 256 terms
    (256 * 2^-24 = 1.5e-5 each at worst), the exponentials (1e-6) and the division: 4e-5 relative"""
    return 0.5 * ulp(ref, 7) + 4e-5 * ref.abs()
