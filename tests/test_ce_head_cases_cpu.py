"""No GPU: the cases of the cross-entropy head's operator tests (tests/ce_head_cases.py, run by test_gpu_ce_head_exact.py) are what
they claim.  The fp64 torch reference agrees with the oracle's own restatement; the kernels' arithmetic, restated in fp32, stays
inside the GPU test's bounds with at least 4x to spare on every case (so a kernel that misses them is wrong, not unlucky); fp32 and
fp64 argmax agree on every pixel (so the GPU test may demand equality); the table reaches every kernel it promises."""
import numpy as np
import pytest
import torch

import ce_head_cases as K

SPARE = 4.0
ALL_VALUES = sorted({c.values for c in K.NHWC_CASES + K.NCHW_CASES}, key=str)


def _ids(v):
    return f"c{v[0]}_{'x'.join(map(str, v[1]))}_{v[2]}_{v[3]}"


def test_reference_agrees_with_the_oracle_where_nothing_is_ignored():
    """seg_step.cross_entropy_np knows no ignored label: compared on the one-hot labels, where every pixel is valid."""
    from oracle import seg_step
    for C, shape, family, weight in [(13, K.SMALL, "ints", "rand"), (19, K.MEDIUM, "far", "rand"), (19, K.MEDIUM, "ints", "zeros"),
                                     (1, K.SMALL, "ints", "rand"), (32, K.SMALL, "far", "none")]:
        v = K.case_values(C, shape, family, weight)
        ref = v["onehot"]
        loss, dl = seg_step.cross_entropy_np(v["x"].numpy(), v["lab"]["y_onehot"].numpy(), None if v["w"] is None else v["w"].numpy())
        assert abs(loss - ref["loss"]) <= 1e-12 * max(1, abs(loss)), (C, family, loss, ref["loss"])
        assert np.abs(dl - ref["dl"].numpy()).max() <= 1e-14
        assert torch.equal(seg_step.predict_torch(v["x"].double()), ref["preds"])
        cm = seg_step.confusion_matrix_np(v["lab"]["y_onehot"].numpy(), ref["preds"].numpy(), C)
        assert np.array_equal(cm, ref["confmat"])
        assert np.array_equal(torch.argmax(v["lab"]["onehot"], 1).numpy(), v["lab"]["y_onehot"].numpy())


@pytest.mark.parametrize("values", ALL_VALUES, ids=_ids)
def test_fp32_arithmetic_stays_inside_the_bounds_with_room_and_argmax_is_unambiguous(values):
    v = K.case_values(*values)
    lab = v["lab"]
    for which, y, valid in (("int", lab["y"], ~lab["ign"]), ("onehot", lab["y_onehot"], torch.ones_like(lab["ign"]))):
        ref = v[which]
        loss, dl, preds = K.kernel_arithmetic_f32(v["x"], y, valid, v["w"])
        le, lb = abs(loss - ref["loss"]), K.loss_bound(ref["loss"])
        de, db = float((dl.double() - ref["dl"]).abs().max()), K.dl_bound(ref["dl"])
        print(f"{_ids(values)} {which}: loss {ref['loss']:.9f} err {le:.2e} (bound {lb:.2e}), dl err {de:.2e} (bound {db:.2e})")
        assert np.isfinite(ref["loss"]) and bool(torch.isfinite(ref["dl"]).all())
        assert le * SPARE <= lb, (which, le, lb)
        assert de * SPARE <= db, (which, de, db)
        assert torch.equal(preds, ref["preds"]), "fp32 and fp64 argmax differ"
        # the far family is far: a typical valid pixel's loss term is near 100
        if values[2] == "far" and values[0] > 1 and values[3] == "none":
            assert ref["loss"] > 40
        # ignored pixels and classes that weigh nothing carry no gradient
        assert float(ref["dl"].permute(0, 2, 3, 1)[~valid].abs().max() if (~valid).any() else 0.0) == 0.0


@pytest.mark.parametrize("values", ALL_VALUES, ids=_ids)
def test_labels_are_what_the_issue_of_each_kind_says(values):
    C, shape = values[0], values[1]
    lab = K.case_values(*values)["lab"]
    ign, y = lab["ign"], lab["y"]
    share = float(ign.float().mean())
    assert 0.08 < share < 0.25, share
    if C > 2:
        assert int((y == K.ABSENT_CLASS).sum()) == 0 and len(torch.unique(y)) == C - 1
    for kind, vals in (("u8", K.IGNORED_U8), ("i32", K.IGNORED_I32), ("i64", K.IGNORED_I64)):
        l64 = lab[kind].to(torch.int64)
        assert torch.equal(l64[~ign], y[~ign])
        assert bool(((l64[ign] < 0) | (l64[ign] >= C)).all())
        assert set(l64[ign].tolist()) == {C if x is None else x for x in vals}
    # the wide values an (int) cast would fold into [0, C): 2^32 + 3 -> 3, -(2^32) + 1 -> 1
    narrowed = lab["i64"].to(torch.int32).to(torch.int64)[ign]
    if C > 3:
        assert bool(((narrowed >= 0) & (narrowed < C)).any())
    assert int(lab["zero"].sum()) == min(K.ZERO_ONEHOT_PIXELS, int((y != 0).sum()))
    assert float(lab["onehot"].permute(0, 2, 3, 1)[lab["zero"]].abs().max() if lab["zero"].any() else 0) == 0
    exact, fits = K.expected_targets(lab["i64"], C)
    assert bool((~fits).any()) and bool(fits[~ign].all())


def test_weights():
    assert K.weight_of(13, "none") is None
    w = K.weight_of(13, "rand")
    assert w[2] == 0 and float(w[w != 0].min()) >= 0.1 and float(w.max()) < 1.1
    z = K.weight_of(19, "zeros")
    assert int((z == 0).sum()) == 7


def test_routing_predicate_and_named_kernels():
    """routes_vec4 restates ce_head(): HW % 4 == 0, NHWC rows no wider than the four-pixel kernel's register row (16 for C <= 16,
    else 32), logits / dlogits_nchw on 16 bytes and preds_u8 on 4."""
    for HW in (116, 117, 768):
        for C in (1, 13, 16, 17, 32):
            for dl_ld in (0, 16, 24, 32):
                if dl_ld and dl_ld < C:
                    continue
                for aligned in (False, True):
                    want = HW % 4 == 0 and aligned and not (dl_ld > 16 and C <= 16)
                    assert K.routes_vec4(HW, C, dl_ld, aligned) == want
    for c in K.NCHW_CASES:
        assert K.nchw_kernel(c.C, c.shape, c.dl_ld, bool(c.misalign)) == c.kernel, c.name
        assert c.dl_ld == 0 or (c.dl_ld >= c.C and c.dl_ld % 8 == 0)
    names = [c.name for c in K.NHWC_CASES] + [c.name for c in K.NCHW_CASES]
    assert len(set(names)) == len(names)


def test_the_table_covers_what_it_promises():
    """All six NHWC instantiations at the small and the medium shape; row strides 16 and 32 past the grid cap; every (C, ld) of
    the issue; both families and a weighted and an unweighted case per row stride; both four-pixel instantiations; the one-pixel
    kernel reached in each of three ways; both store_row types (through either entry) at 16 / 24 / 32."""
    assert {(c.C, c.ld) for c in K.NHWC_CASES} == set(K.C_LD)
    for C, ld in K.C_LD:
        assert {c.shape for c in K.NHWC_CASES if (c.C, c.ld) == (C, ld)} >= {K.SMALL, K.MEDIUM}
    seen = {(c.kernel(dt), c.shape) for c in K.NHWC_CASES for dt in K.DTYPES}
    for dt in K.DTYPES:
        for ld in (16, 24, 32):
            assert {(f"nhwc_{dt}_{ld}", K.SMALL), (f"nhwc_{dt}_{ld}", K.MEDIUM)} <= seen
        assert {(f"nhwc_{dt}_16", K.LARGE), (f"nhwc_{dt}_32", K.LARGE)} <= seen
    large = [c for c in K.NHWC_CASES if c.shape == K.LARGE]
    assert len(large) == 2 and all(c.ld in (16, 32) for c in large) and not any(c.shape == K.LARGE for c in K.NCHW_CASES)
    for ld in (16, 24, 32):
        mine = [c for c in K.NHWC_CASES if c.ld == ld]
        assert {c.family for c in mine} == {"ints", "far"} and {"none", "rand"} <= {c.weight for c in mine}
    assert any(c.weight == "zeros" for c in K.NHWC_CASES) and any(c.weight == "zeros" for c in K.NCHW_CASES)
    # shapes: a partly filled single block, several blocks, more pixels than the capped grid has threads
    B, H, W = K.SMALL
    assert B * H * W < 256 and (H * W) % 4
    B, H, W = K.MEDIUM
    assert K.blocks(B * H * W) == 9 and (H * W) % 4 == 0
    B, H, W = K.LARGE
    assert B * H * W > K.CE_BLOCK_CAP * 256 and K.blocks(B * H * W) == K.CE_BLOCK_CAP
    kernels = {c.kernel for c in K.NCHW_CASES}
    assert kernels == {"main4_16", "main4_32", "scalar_odd_hw", "scalar_dl_ld", "scalar_misaligned"}
    assert {c.misalign for c in K.NCHW_CASES if c.misalign} == {"logits", "preds", "dlogits"}
    # store_row<float> and <bf16_t> at each row stride from the four-pixel and from the one-pixel kernel
    for ld in (16, 24, 32):
        fams = {c.kernel.split("_")[0] for c in K.NCHW_CASES if c.dl_ld == ld}
        assert fams == {"main4", "scalar"}, (ld, fams)
    # each misaligned case repeats an aligned one on the same values
    for c in K.NCHW_CASES:
        if c.misalign:
            assert any(a.values == c.values and a.dl_ld == c.dl_ld and not a.misalign and a.kernel.startswith("main4") for a in K.NCHW_CASES)
    # layouts: every NCHW case's (C, dl_ld) is an NHWC (C, ld), so both entries can run on the same values
    for c in K.NCHW_CASES:
        if c.dl_ld:
            assert (c.C, c.dl_ld) in K.C_LD, c.name


def test_jaccard_matrices_are_the_edges_they_claim():
    m = K.jaccard_matrices()
    assert m["c1"].shape == (1, 1) and m["c32"].shape == (32, 32)
    assert int(m["zeros"].abs().sum()) == 0
    a = m["absent"]
    assert int(a[3].sum()) == 0 and int(a[:, 3].sum()) == 0 and int(a[7].sum()) == 0 and int(a[:, 7].sum()) > 0
    assert int(m["near_2pow40"].min()) > 2 ** 39 and int(m["prefilled_2pow40"].min()) >= 2 ** 40
    assert all(v.dtype == torch.int64 for v in m.values())
