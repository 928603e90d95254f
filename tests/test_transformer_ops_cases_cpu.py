"""No GPU: the references of tests/transformer_cases.py equal the installed transformers / torch.nn modules in fp64, every case
declared exact is inside the exact range on its reference alone, and every case written for a loop or a cap gives more than
one trip (or the intended group size) by the restated launch arithmetic."""
import math

import pytest
import torch
import torch.nn.functional as F

import transformer_cases as T

PIN = 1e-12


def _close(a, b, tol=PIN):
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    err = float((a - b).abs().max() / (b.abs().max() + 1e-300))
    assert err <= tol, err


# ------------------------------------------------------------------------------------------------ restatements vs the library
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("grid", T.SWIN_GRIDS + [(9, 5)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_window_attention_restatement_equals_transformers(grid, shift):
    """SwinAttention fed by maybe_pad / cyclic_shift / window_partition / get_attn_mask on the padded, rolled grid, then
    window_reverse, the reverse shift and the crop — SwinLayer.forward with always_partition (the backbone's mode: grids smaller
    than one window are padded, the window is not clamped), without the norms and the MLP around it."""
    from transformers import SwinConfig
    from transformers.models.swin import modeling_swin as M
    H, W = grid
    heads, B = 2, 2
    C = 32 * heads
    torch.manual_seed(H * 100 + W + shift)
    cfg = SwinConfig(embed_dim=C, depths=[2], num_heads=[heads], window_size=7)
    cfg._attn_implementation = "sdpa"   # (the eager interface takes its softmax in fp32 whatever the input dtype)
    layer = M.SwinLayer(cfg, C, (H, W), heads, shift_size=shift).double().eval()
    att = layer.attention
    with torch.no_grad():
        for lin in (att.q_proj, att.k_proj, att.v_proj):
            lin.bias.normal_()
        att.relative_position_bias.relative_position_bias_table.normal_()
        att.o_proj.weight.copy_(torch.eye(C))
        att.o_proj.bias.zero_()
        x = torch.randn(B, H, W, C, dtype=torch.float64)
        hs, pad = layer.maybe_pad(x, H, W)
        Hp, Wp = hs.shape[1:3]
        wins = M.window_partition(layer.cyclic_shift(hs), 7).view(-1, 49, C)
        mask = layer.get_attn_mask(Hp, Wp, dtype=hs.dtype, device=hs.device)
        assert (mask is None) == (shift == 0)
        out, _ = att(wins, mask)
        out = layer.cyclic_shift(M.window_reverse(out.view(-1, 7, 7, C), 7, Hp, Wp), reverse=True)[:, :H, :W]
        qkv = torch.cat([att.q_proj(x), att.k_proj(x), att.v_proj(x)], -1)
        bias = torch.cat([att.q_proj.bias, att.k_proj.bias, att.v_proj.bias])
        table = att.relative_position_bias.relative_position_bias_table
        _close(T.window_attention_ref(qkv, bias, table, heads, shift), out)


def test_rel_index_and_region_labels_are_the_librarys():
    from transformers.models.swin import modeling_swin as M
    rp = M.SwinRelativePositionBias(1, (7, 7))
    assert torch.equal(T.rel_index().reshape(-1), rp.relative_position_index)


def test_sf_attention_restatement_equals_transformers():
    """SegformerAttention (sequence reduction 1, identity output projection) fed by the states; the restatement by its q / k / v"""
    from transformers import SegformerConfig
    from transformers.models.segformer import modeling_segformer as S
    torch.manual_seed(3)
    hid, heads, B, N = 128, 2, 2, 48
    cfg = SegformerConfig()
    cfg._attn_implementation = "sdpa"   # (the eager interface takes its softmax in fp32 whatever the input dtype)
    att = S.SegformerAttention(cfg, hid, heads, 1).double().eval()
    assert att.head_dim == 64 and att.scaling == 0.125
    with torch.no_grad():
        att.o_proj.weight.copy_(torch.eye(hid))
        att.o_proj.bias.zero_()
        x = torch.randn(B, N, hid, dtype=torch.float64)
        out, _ = att(x, 6, 8)
        q, k, v = att.q_proj(x), att.k_proj(x), att.v_proj(x)
        ref = T.sf_attention_ref(q, k, v)
        _close(ref, out)
        qh, kh, vh = (t.view(B, -1, heads, 64).transpose(1, 2) for t in (q, k, v))
        _close(ref, (torch.softmax(qh @ kh.transpose(-1, -2) / 8, -1) @ vh).transpose(1, 2).reshape(B, N, hid))


@pytest.mark.parametrize("C,H,W", [(64, 8, 8), (128, 8, 16), (64, 5, 7)])
def test_mix_ffn_restatement_equals_transformers(C, H, W):
    """SegformerMixMLP with layernorm_after in front and the residual behind it (SegformerLayer.forward's second half)"""
    from transformers import SegformerConfig
    from transformers.models.segformer import modeling_segformer as S
    torch.manual_seed(C + H)
    cfg = SegformerConfig(hidden_act="gelu", hidden_dropout_prob=0.0)
    mlp = S.SegformerMixMLP(cfg, C, 4 * C).double().eval()
    ln = torch.nn.LayerNorm(C, eps=1e-6).double()
    ln2 = torch.nn.LayerNorm(C, eps=1e-6).double()
    with torch.no_grad():
        for m in (ln, ln2):
            m.weight.normal_()
            m.bias.normal_()
        x = torch.randn(2, H, W, C, dtype=torch.float64)
        t = x.view(2, H * W, C)
        out = (mlp(ln(t), H, W) + t).view(2, H, W, C)
        p = dict(ln_g=ln.weight, ln_b=ln.bias, w1=mlp.fc1.weight, b1=mlp.fc1.bias, dw_w=mlp.dwconv.dwconv.weight[:, 0],
                 dw_b=mlp.dwconv.dwconv.bias, w2=mlp.fc2.weight, b2=mlp.fc2.bias)
        got, got_ln = T.mix_ffn_ref(x, p, 1e-6, ln2=(ln2.weight, ln2.bias))
        _close(got, out)
        _close(got_ln, ln2(out))
        pre, act = T.dwconv_gelu_ref(x, p["dw_w"][:C], p["dw_b"][:C])
        _close(act, F.gelu(pre))


def test_decode_head_restatement_equals_transformers():
    from transformers import SegformerConfig
    from transformers.models.segformer import modeling_segformer as S
    torch.manual_seed(11)
    hs, D, labels, B, H, W = [16, 24, 40, 64], 32, 5, 2, 16, 32
    cfg = SegformerConfig(hidden_sizes=hs, decoder_hidden_size=D, num_labels=labels, classifier_dropout_prob=0.0)
    head = S.SegformerDecodeHead(cfg).double().eval()
    with torch.no_grad():
        bn = head.batch_norm
        for t in (bn.weight, bn.bias, bn.running_mean):
            t.normal_()
        bn.running_var.uniform_(0.5, 2.0)
        feats = [torch.randn(B, H >> i, W >> i, hs[i], dtype=torch.float64) for i in range(4)]
        want = head([f.permute(0, 3, 1, 2).contiguous() for f in feats])
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        shift = bn.bias - bn.running_mean * scale
        got = T.decode_head_ref(feats, [m.proj.weight for m in head.linear_projections], [m.proj.bias for m in head.linear_projections],
                                head.linear_fuse.weight[:, :, 0, 0], scale, shift, head.classifier.weight[:, :, 0, 0], head.classifier.bias)
        _close(got, want)


def test_pool_resize_layernorm_restatements_equal_torch():
    torch.manual_seed(5)
    for (h, w, H, W) in [(1, 1, 2, 2), (2, 3, 4, 6), (3, 5, 12, 20), (1, 1, 4, 4), (2, 2, 16, 16), (3, 3, 4, 4), (6, 6, 4, 4), (6, 6, 16, 16),
                         (5, 7, 8, 9), (4, 8, 32, 64)]:
        x = torch.randn(2, h, w, 3, dtype=torch.float64)
        want = F.interpolate(x.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        _close(T.bilinear_ref(x, H, W), want)
    for n in (2, 4, 7, 16):
        for S in (1, 2, 3, 6):
            x = torch.randn(2, n, n, 3, dtype=torch.float64)
            _close(T.avgpool_ref(x, S), torch.nn.AdaptiveAvgPool2d(S)(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1))
    for eps in (1e-5, 1e-6):
        ln = torch.nn.LayerNorm(96, eps=eps).double()
        with torch.no_grad():
            ln.weight.normal_()
            ln.bias.normal_()
            x = 100 + torch.randn(7, 96, dtype=torch.float64)
            _close(T.layernorm_ref(x, ln.weight, ln.bias, eps), ln(x))


def test_patch_merge_restatement_equals_transformers():
    from transformers import SwinConfig
    from transformers.models.swin import modeling_swin as M
    torch.manual_seed(9)
    B, H, W, C = 2, 4, 6, 16
    pm = M.SwinPatchMerging(C).double().eval()
    del SwinConfig
    with torch.no_grad():
        pm.norm.weight.normal_()
        pm.norm.bias.normal_()
        x = torch.randn(B, H, W, C, dtype=torch.float64)
        want = pm(x.view(B, H * W, C), (H, W))
        got = T.patch_merge_ref(x, pm.norm.weight, pm.norm.bias, pm.norm.eps).view(B, -1, 4 * C) @ pm.reduction.weight.T
        _close(got, want)


# ------------------------------------------------------------------------------------------- exact cases, on the reference alone
@pytest.mark.parametrize("case", T.SF_GATHER_CASES, ids=lambda c: c[0])
def test_sf_gather_case_is_a_gather(case):
    name, dt, att2, B, heads, N, Nk, _ = case
    q, kv, want, tgt = T.sf_gather_inputs(case)
    hid = 64 * heads
    for t in (q, kv, want):
        assert torch.equal(T.bf16r(t), t)
    assert float(want.abs().min()) >= 1 and float(want.abs().max()) <= 255
    nq = min(N, 64)                               # the scores of the first queries: winner 512, every loser <= 384
    s = torch.einsum("bqhc,bkhc->bhqk", q[:, :nq].view(B, nq, heads, 64), kv[:, :, :hid].reshape(B, Nk, heads, 64)) / 8
    top = s.gather(-1, tgt[:, :, :nq, None])
    assert torch.equal(top, torch.full_like(top, 512.0))
    s.scatter_(-1, tgt[:, :, :nq, None], -1e9)
    assert float(s.max()) <= 512 - 128
    assert math.exp(-104) < 2.0 ** -149 and 128 * math.log2(math.e) > 150   # every loser's exp / exp2 is exactly 0 in fp32
    if N <= 256:
        _close(T.sf_attention_ref(q, kv[..., :hid], kv[..., hid:]), want, 1e-15)
    two_tile = dt == "bf16" and att2 == 1
    qb, gx, breaks, ragged = T.att_walk(two_tile, B, heads, N)
    assert qb == T.SF_WALKED.get(name, 1), (name, qb)
    if name in ("walk2_two_tile", "walk2_one_tile", "walk2_f32"):
        assert breaks and ragged and gx > 1


@pytest.mark.parametrize("decoys", [False, True], ids=["gather", "mask"])
@pytest.mark.parametrize("case", T.SWIN_GATHER_CASES, ids=lambda c: c[0])
def test_swin_gather_case_is_a_gather(case, decoys):
    name, B, H, W, heads, shift = case
    if decoys and shift == 0:
        return
    qkv, bias, want, ndec = T.swin_gather_inputs(case, decoys)
    for t in (qkv, bias, want):
        assert torch.equal(T.bf16r(t), t)
    assert float(want.abs().min()) >= 1
    assert 64 * 10 * 32 ** -0.5 > 104 + 9          # one differing bit costs 113.1
    table = torch.zeros(169, heads, dtype=torch.float64)
    ref = T.window_attention_ref(qkv, bias, table, heads, shift)
    assert float((ref - want).abs().max()) < 255 * math.exp(-43), float((ref - want).abs().max())
    if decoys:
        tok, lab = T.window_slots(H, W, shift)
        straddle = sum(1 for wi in range(tok.shape[0]) if len({int(l) for l, t in zip(lab[wi], tok[wi]) if t >= 0}) > 1)
        # every window whose real tokens straddle regions has a query whose decoy must lose; the table as a whole has queries
        # whose decoy must win (with the mask at -inf those would lose: the cases tell -100 from -inf).  2 x 2 and 8 x 16 have no
        # such window: the pad tokens lie between their regions
        assert ndec[0] == straddle and ndec[1] <= straddle and (straddle >= 1) == (name in T.SWIN_MASK_NAMES)
        if straddle:
            assert ndec[1] >= 1
    else:
        assert ndec == [0, 0]


@pytest.mark.parametrize("case", T.HEAD_CASES, ids=str)
def test_head_case_is_exact(case):
    d = T.head_inputs(case)
    z, logits = T.check_head_exact(d)
    assert torch.equal(T.bf16r(z), z) and torch.equal(logits.float().double(), logits)
    for k in ("f0", "w0", "g1", "g2", "g3", "wc"):
        assert torch.equal(T.bf16r(d[k]), d[k])
    assert T.head_core_ref(**d, round_z=True)[1].equal(logits)


def test_wint_closed_form_is_dyadic_and_sums_to_one_per_stage():
    m = T.wint_ref()
    assert torch.equal(T.bf16r(m), m)
    for lo, hi in ((0, 60), (60, 84), (84, 96)):
        assert torch.equal(m[:, lo:hi].sum(1), torch.ones(128, dtype=torch.float64))


@pytest.mark.parametrize("case", T.GEMM_CASES, ids=lambda c: c[0])
def test_gemm_case_is_exact(case):
    name, (N, H, W), Cin, Cout, R, stride, pad = case
    x, w, b = T.gemm_inputs(case)
    y = F.conv2d(x, w, b, stride=stride, padding=pad)
    assert float(y.abs().max()) <= 256 and float(y.abs().max()) >= 8
    assert float(F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride, padding=pad).max()) < 2 ** 24


def test_pool_cases_have_power_of_two_bins():
    for n in (4, 2):
        for S in (1, 2, 3, 6):
            assert all(c in (1, 2, 4) for c in T.pool_bins(n, S)), (n, S)
    assert T.pool_bins(4, 3) == [2, 2, 2] and T.pool_bins(4, 6) == [1, 2, 1, 1, 2, 1] and T.pool_bins(4, 2) == [2, 2]


@pytest.mark.parametrize("case", T.DW_CASES, ids=lambda c: c[0])
def test_dw_case_preactivation_is_exact_and_takes_its_body(case):
    name, B, H, W, C, lmax, _ = case
    x, w, b = T.dw_inputs(case)
    pre, _ = T.dwconv_gelu_ref(x, w, b)
    assert float(pre.abs().max()) <= 256 and torch.equal(pre, pre.round())
    for dt in T.DTYPES:
        L, cg, gx, gy, trips = T.dw_launch(dt, B, H, W, C, lmax)
        assert W % L == 0
        if lmax:
            assert L == lmax
        if name.startswith("cap"):
            assert gx == 8192 and trips == 2 and B * H * (W // L) % (gx * (256 // cg)) != 0
        else:
            assert trips == 1
    # the table reaches every body in both dtypes, one group / 64 per workgroup / 5 workgroups in y, and a one-row image
    for dt in T.DTYPES:
        assert {T.dw_launch(dt, c[1], c[2], c[3], c[4], c[5])[0] for c in T.DW_CASES} == {1, 2, 4, 8, 16}
    assert {T.dw_launch("f32", c[1], c[2], c[3], c[4], c[5])[0] for c in T.DW_CASES if c[5] == 0} == {1, 2, 4, 8, 16}
    assert {T.dw_launch("bf16", c[1], c[2], c[3], c[4], c[5])[1:4:2] for c in T.DW_CASES} >= {(1, 1), (64, 1), (64, 5)}


def test_elementwise_loop_cases_loop_with_a_ragged_last_trip():
    for name, c in T.EW_LOOP.items():
        n = c["chunks"]
        trips, last = T.ew_trips(n)
        assert n > 1048576 and (n - 1048576) % 256 != 0 and trips == 2 and 0 < last < 1048576, name
    c = T.EW_LOOP["swin_avgpool"]
    assert c["chunks"] == c["B"] * c["S"] ** 2 * (c["C"] // 8)
    c = T.EW_LOOP["sf_upsample_sum_bn_relu"]
    assert c["H"] % 8 == 0 and c["W"] % 8 == 0 and c["chunks"] == c["B"] * c["H"] * c["W"] * c["D"] // 8
    for k in ("swin_bilinear_add", "sf_bilinear_nhwc"):
        c = T.EW_LOOP[k]
        assert c["chunks"] == c["B"] * 2 * c["h"] * 2 * c["w"] * c["C"] // 8
    # the largest bf16 launch of the network tests is exactly the cap: one short of looping
    assert T.ew_trips(128 * 128 * 512 // 8) == (1, 1048576)


def test_layernorm_cases_reach_their_group_sizes():
    assert [T.sf_ln_group("f32", c) for c in T.SF_LN_C] == [16, 32, 64, 64]
    assert [T.sf_ln_group("bf16", c) for c in T.SF_LN_C] == [8, 16, 64, 64]
    assert T.sf_ln_group("f32", 516) is None and T.sf_ln_group("bf16", 1032) is None and T.sf_ln_group("bf16", 1024) == 64
    assert [T.swin_ln_group("f32", c) for c in T.SWIN_LN_C] == [(16, 2), (16, 3), (16, 6), (32, 6)]
    assert [T.swin_ln_group("bf16", c) for c in T.SWIN_LN_C] == [(16, 1), (16, 2), (16, 3), (16, 6)]
    assert [T.swin_ln_group("f32", 4 * c) for c in T.MERGE_C] == [(16, 6), (64, 6), None]   # all six chunks per lane; refused
    assert [T.swin_ln_group("bf16", 4 * c) for c in T.MERGE_C] == [(16, 3), (32, 6), (64, 6)]
    g = T.gen(0)
    for eps_kind in ("tinyvar_eps1e-5", "tinyvar_eps1e-6"):
        x, eps = T.ln_rows(eps_kind, 8, 96, g)
        one = torch.ones(96, dtype=torch.float64)
        a, b = T.layernorm_ref(x, one, 0 * one, 1e-5), T.layernorm_ref(x, one, 0 * one, 1e-6)
        assert float((a - b).abs().max() / b.abs().max()) > 0.2     # the wrong eps is a change of tens of percent


def test_case_names_are_unique():
    for table in (T.SF_GATHER_CASES, T.SWIN_GATHER_CASES, T.DW_CASES, T.GEMM_CASES):
        names = [c[0] for c in table]
        assert len(set(names)) == len(names)


def test_denominator_case_tells_rounded_from_unrounded():
    """the expected output of T.denominator_inputs is the rounding-faithful reference, and a kernel that took the softmax
    denominator from the rounded P (or rounded neither) would be outside the bound in every element"""
    q, kv, want, c = T.denominator_inputs()
    hid = q.shape[-1]
    for t in (q, kv):
        assert torch.equal(T.bf16r(t), t)
    ref = T.sf_attention_ref(q, kv[..., :hid], kv[..., hid:], round_p=True)
    _close(ref, want, 1e-14)
    x = torch.tensor(math.exp(-2.0), dtype=torch.float64)
    lo = T.bf16r(x) - T.ulp(x, 7)
    assert T.bf16r(x) > x and 0.55 < float((x - lo) / T.ulp(x, 7)) < 0.62          # rounds up, 0.08 ulp from the tie
    bound = T.denominator_bound(want)
    assert float(((c - want[0, 0]).abs() / bound[0, 0]).min()) > 1.3
    plain = T.sf_attention_ref(q, kv[..., :hid], kv[..., hid:])
    assert float(((plain - want).abs() / bound).min()) > 1.3
