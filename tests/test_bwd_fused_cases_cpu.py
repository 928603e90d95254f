"""No GPU: every case of the fused-backward operator tests (tests/bwd_fused_cases.py, run by test_gpu_bwd_fused_exact.py) is inside
the exact range — checked on its fp64 reference alone — is dispatched to the kernel family it names according to the restated
predicates of exact_cases.py, and, where it is meant to loop, gives a persistent workgroup more than one tile, unevenly."""
import pytest
import torch

import bwd_fused_cases as B
import exact_cases as E


def test_case_names_are_unique_and_every_switch_has_a_default():
    names = ([c.name for c in B.BNR_CASES] + [c.name for c in B.BN_CASES] + [c.name for c in B.PARITY_CASES]
             + [c.name for c in E.CONV_CASES + E.FUSED_CASES])
    assert len(set(names)) == len(names)
    for c in B.BNR_CASES:
        assert set(dict(c.tune)) <= set(E.TUNE_DEFAULTS), c.name
    assert {n for n, _ in B.CHAIN_CASES} <= set(B.BNR_BY_NAME)


@pytest.mark.parametrize("case", B.BNR_CASES, ids=lambda c: c.name)
def test_bnr_case_is_exact_and_goes_where_it_is_meant_to(case):
    B.check_bnr_range(case, B.bnr_reference(case))
    loops = B.check_bnr_dispatch_and_loops(case)
    assert bool(loops) == case.loops, (case.name, loops)
    for dt in E.DTYPES:
        if case.tune or case.launch(dt)[0].startswith("hg_") or case.N * case.H * case.W // 256 <= 256:
            assert case.grid_rows(dt) is not None


def test_the_bnr_table_covers_what_it_promises():
    """Every tile shape of the 64-wide halo-GEMM and the 128-wide one, a column block with n0 > 0 for each width, the XCD remap with
    a quotient and a remainder, both mask sources, masked stores, the pooled forms with skip columns, and a persistent grid that
    walks 3 and 2 tiles per workgroup."""
    shapes, n0, remap, kinds = set(), set(), set(), set()
    for c in B.BNR_CASES:
        fam = c.launch("bf16")[0]
        assert fam == c.launch("f32")[0]
        if fam.startswith("hg_"):
            tw, th, bn = E.hg_shape(c.H, c.W, c.Cout)
            nwork = c.grid_rows("bf16") * (c.Cout // bn)
            shapes.add((tw, th, bn))
            if c.Cout > bn:
                n0.add(bn)
            if nwork >= 9 and nwork % 8:
                remap.add(bn)
        kinds.add((fam.split("_")[0], c.from_out, c.bnr_mask, bool(c.pool_c0), c.pool_c0 not in (0, c.Cout), c.accumulate, c.acc_src))
        if c.loops:
            assert B.check_bnr_dispatch_and_loops(c)["bf16"][2:] == (3, 2)
    assert {(32, 8, 64), (16, 16, 64), (16, 8, 64), (16, 8, 128)} <= shapes
    assert n0 == {64, 128} and remap == {64, 128}
    has = lambda **kw: any(all(dict(zip(("fam", "from_out", "mask", "pool", "partial_pool", "acc", "acc_src"), k))[a] == v for a, v in kw.items())
                           for k in kinds)
    assert has(fam="hg", from_out=True, acc=True) and has(fam="hg", mask=True, acc_src=True) and has(fam="hg", partial_pool=True, mask=True)
    assert has(fam="hg", pool=True, acc=True) and has(fam="halo", pool=True) and has(fam="halo", pool=False)


def test_bnr_refusals_are_what_the_restated_dispatch_refuses():
    """The shapes of test_bnr_refusals: the restated launch_conv refuses them too (an AssertionError of conv_kernel)."""
    ck = lambda **kw: E.conv_kernel("f32", 1, kw.pop("H", 16), kw.pop("W", 64), 16, 64, kw.pop("C0", 16), 0, kw.pop("Cout", 16), 3, 1, 1, 1, **kw)
    with pytest.raises(AssertionError):
        E.conv_kernel("f32", 1, 10, 12, 10, 12, 64, 0, 64, 3, 1, 1, 1, bnr=True)           # gather-form shape
    with pytest.raises(AssertionError):
        ck(bnr=True, bnr_mask=True)                                                        # small-channel kernel: no masked store
    with pytest.raises(AssertionError):
        ck(bnr=True, bnr_out=True)                                                         # ... and no mask from `out`
    with pytest.raises(AssertionError):
        E.conv_kernel("f32", 1, 24, 96, 24, 96, 64, 0, 64, 3, 1, 1, 1, bnr_mask=True)      # masked store without the reduction
    with pytest.raises(AssertionError):
        E.conv_kernel("f32", 1, 24, 96, 24, 96, 64, 0, 64, 3, 1, 1, 1, bnr=True, in_scale=True)
    assert not E.hg_applicable("bf16", 128, 0, 32, 3, 1, 1, 1, 24, 96, 24, 96, True, False, bnr=True)
    assert E.hg_applicable("bf16", 128, 0, 32, 3, 1, 1, 1, 24, 96, 24, 96, True, False)


@pytest.mark.parametrize("case", B.BN_CASES, ids=lambda c: c.name)
def test_bn_case_is_made_of_dyadic_rationals(case):
    r = B.bn_reference(case)           # (asserts on every intermediate while it builds the reference)
    assert case.rows & (case.rows - 1) == 0
    for k in ("dgamma", "dbeta", "coef", "dy"):
        assert torch.equal(r[k].float().double(), r[k]), (case.name, k)
    B.check_mask_variety(case.name, r["y"].t().reshape(1, case.C, case.rows, 1), r["scale"], r["shift"])
    if case.mask == "out":
        my = (r["y"].double() * r["scale"].double() + r["shift"].double() > 0).double()
        assert float((my != (r["out"] > 0).double()).double().mean()) > 0.2
    if case.pre_nblk:
        assert not case.accumulate_param
        assert torch.equal(r["partial"].sum(2), torch.stack([r["dbeta"], (r["dz"] * r["y"].double()).sum(0)]))
    assert float(r["dy"].abs().max()) <= 256
    if case.dres:
        assert float(r["dres"].abs().max()) <= 256


def test_bn_table_covers_what_it_promises():
    cs = B.BN_CASES
    assert {c.C for c in cs} == {16, 64, 512} and {c.rows for c in cs} == {1024, 2 ** 14}
    assert {c.pre_nblk for c in cs} == {0, 1, 9, 640} and {c.mask for c in cs} == {"out", "mscale", "none", "premasked"}
    assert {c.dres for c in cs} == {"", "write", "accumulate"} and any(c.accumulate_param for c in cs) and any(not c.want_dy for c in cs)
    assert all(c.pre_nblk > 0 for c in cs if c.mask == "premasked")


@pytest.mark.parametrize("name,how", B.CHAIN_CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_chain_case_parameter_gradients_are_exact(name, how):
    c = B.BNR_BY_NAME[name]
    b = B.chain_reference(name)
    assert (how == "premasked") == c.bnr_mask and (how == "out") == c.from_out
    for k in ("dgamma", "dbeta"):
        assert torch.equal(b[k].float().double(), b[k])
    assert b["pow2"] == (name == "bnr_p16to16_small")


@pytest.mark.parametrize("case", B.PARITY_CASES, ids=lambda c: c.name)
def test_parity_case_is_exact_and_runs_the_gather_form_kernel(case):
    B.check_parity_case(case, B.parity_reference(case))


def test_parity_table_covers_what_it_promises():
    cs = B.PARITY_CASES
    px = {c.name: c.N * c.Ho * c.Wo for c in cs}
    assert px["par_64to128_35px"] < 128 and px["par_64to128_35px"] % 32
    assert px["par_128to256_720px"] > 128 and px["par_128to256_720px"] % 128 and B.PARITY_CASES[1].N > 1
    assert px["par_16to64_256row_tiles"] > 256 and px["par_16to64_256row_tiles"] % 256
    assert any(c.R == 1 and c.accumulate for c in cs) and any(c.R == 3 and c.accumulate for c in cs)
    assert {c.launch(dt)[1].split("_")[-1] for c in cs for dt in E.DTYPES} >= {"128x128", "128x64", "256x16"}


def test_pack_table_hits_every_branch_and_every_kind_of_padding():
    B.check_pack_table()


def test_pack_formula_against_plain_indexing():
    """pack_expected itself, element by element, on two small descriptors (forward with a tap subset, transposed)."""
    descs, nfl, _ = B.pack_table("f32")
    p = B.pack_params(nfl)
    for d in (descs[5], descs[7], descs[-1]):
        w = p[d["w_off"]:d["w_off"] + d["Cout"] * d["Cin"] * d["R"] * d["S"]].view(d["Cout"], d["Cin"], d["R"], d["S"])
        e = B.pack_expected(d, p)
        taps = ([(d["r0"] + i * d["rstep"], d["s0"] + j * d["sstep"]) for i in range(d["Rc"]) for j in range(d["Sc"])] if d["Rc"]
                else [(r, s) for r in range(d["R"]) for s in range(d["S"])])
        n = 0
        for row in range(d["rows_pad"]):
            for col in range(d["Kpad"]):
                tp, c = divmod(col, d["Cin_p"])
                v = 0.0
                if tp < len(taps):
                    r, s = taps[tp]
                    if d["tf"] and row < d["Cin"] and c < d["Cout"]:
                        v = float(w[c, row, d["R"] - 1 - r, d["S"] - 1 - s])
                    if not d["tf"] and row < d["Cout"] and c < d["Cin"]:
                        v = float(w[row, c, r, s])
                assert e[row, col] == v, (d["name"], row, col)
                n += v != 0
        assert n > 0


def test_elementwise_shapes_pass_their_thresholds():
    B.check_elementwise_shapes()


@pytest.mark.parametrize("shape", B.STEM_CASES, ids=lambda s: "x".join(map(str, s)))
def test_stem_case_is_exact_and_runs_the_stem_kernel(shape):
    r = B.stem_reference(shape)
    k = B.check_stem_dispatch(shape)
    assert k[2]["ntiles"] == shape[0] * shape[1] * shape[2] // 128
    assert torch.equal(r["staged"].to(torch.bfloat16).double(), r["staged"])
    B.check_mask_variety("stem", r["y"], r["scale"], r["shift"])
