"""No GPU: every case of the rounding tests (tests/rounding_cases.py, run by test_gpu_rounding_exact.py) holds its conditions, checked
on the fp64 references alone.  A case that misses one is a failure, never a skip.

  * every input tensor survives .to(bfloat16) unchanged;
  * every summed quantity (accumulator, statistics, the four-way pool sum, dw, both fused BatchNorm-backward sums) has its sum of
    magnitudes below 2^24 in its own unit, so fp32 holds it exactly in any order;
  * at least 1 % of the stored elements change under the bf16 rounding, upward, downward and on exact ties;
  * the case discriminates: with statistics / partial sums taken from unrounded values at least half of the channels differ; with
    one rounding at the end instead of two at least 0.5 % (accumulate, both epilogue outputs), 2 % (pool) of the elements or one
    weight (lazy input, stem) differ; truncation toward zero instead of round-to-nearest-even differs at every store;
  * the restated dispatch sends the case to the family it names, in both dtypes.
acc_src, bnr_mask and bnr_out exist only in the halo-GEMM (launch_conv refuses them elsewhere: test_gpu_ops_exact.py and
test_gpu_bwd_fused_exact.py assert the refusals), so the small-channel families have no case of those forms."""
import pytest
import torch

import rounding_cases as R


@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c.name)
def test_conv_rounding_case_holds_its_conditions(case):
    print(case.name, R.check_conv_case(case))


@pytest.mark.parametrize("case", R.BNR_CASES, ids=lambda c: c.name)
def test_bnr_rounding_case_holds_its_conditions(case):
    print(case.name, R.check_bnr_case(case))


@pytest.mark.parametrize("case", R.WLAZY_CASES, ids=lambda c: c.name)
def test_wgrad_lazy_rounding_case_holds_its_conditions(case):
    print(case.name, R.check_wlazy_case(case))


def test_parity_stem_and_elementwise_cases_hold_their_conditions():
    print(R.check_parity_case(), R.check_stem_case(), R.check_elementwise())


def test_every_listed_family_has_a_bf16_case_of_every_form():
    fams = lambda form: {c.want("bf16") for c in R.CONV_CASES if c.form == form}
    assert fams("fwd") >= {"hg_n64", "hg_n128", "hg_n32", "halo_p", "halo", "halo_pm", "igemm", "stem"}
    assert fams("epilogue") >= {"hg_n64", "halo_p", "igemm_bm32"}
    for form in ("accumulate", "pool"):
        assert fams(form) >= {"hg_n64", "hg_n128", "halo_p"}, form
    assert fams("acc_src") >= {"hg_n64", "hg_n128"}                 # (the small-channel kernels refuse acc_src)
    assert fams("lazy") >= {"hg_n64", "halo_p", "halo_pm"} and {c.C0 for c in R.CONV_CASES if c.want("bf16") == "halo_p" and c.form == "lazy"} == {16, 32}
    assert {c.want("bf16") for c in R.BNR_CASES} >= {"hg_n64", "hg_n128", "halo_p"}
    assert {(c.from_out, c.bnr_mask, bool(c.pool_c0)) for c in R.BNR_CASES} >= {(False, False, False), (True, False, False), (False, True, False),
                                                                                (True, True, False), (False, False, True), (False, True, True)}
    assert {c.want("bf16") for c in R.WLAZY_CASES} == {"halo", "big_kg1", "big_kg2"}
    names = [c.name for c in R.CONV_CASES + R.BNR_CASES + R.WLAZY_CASES]
    assert len(set(names)) == len(names)
    for c in R.CONV_CASES + R.BNR_CASES:                            # one or two tiles
        assert c.N * c.H * c.W <= 512, c.name


def test_the_store_report_tells_ties_and_directions():
    t = torch.tensor([257.0, 259.0, 256.5, 257.5, 300.0, -257.0, 1.0, 0.0])     # 257 -> 256 (tie, down), 259 -> 260 (tie, up), 256.5 down, 257.5 up
    rep = R.store_report(t)
    assert rep == {"changed": 5 / 8, "up": 2, "down": 3, "ties": 3}, rep
    assert torch.equal(R.rne(t), torch.tensor([256.0, 260, 256, 258, 300, -256, 1, 0], dtype=torch.float64))
    assert torch.equal(R.trunc(t), torch.tensor([256.0, 258, 256, 256, 300, -256, 1, 0], dtype=torch.float64))
