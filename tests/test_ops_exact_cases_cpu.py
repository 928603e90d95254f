"""No GPU: every case of the exact-arithmetic operator tests (tests/exact_cases.py, run by test_gpu_ops_exact.py) is inside
the exact range — checked on its fp64 reference alone — goes to the kernel family it is written for according to the restated
dispatch predicates, and, where it is meant to loop, gives a persistent workgroup more than one tile, unevenly."""
import pytest

import exact_cases as E


@pytest.mark.parametrize("case", E.CONV_CASES, ids=lambda c: c.name)
def test_conv_case_is_exact_and_goes_where_it_is_meant_to(case):
    E.check_exact_range(case, E.case_reference(case))
    loops = E.check_dispatch_and_loops(case)
    assert bool(loops) == bool(case.loops), (case.name, loops)


@pytest.mark.parametrize("case", E.FUSED_CASES, ids=lambda c: c.name)
def test_fused_case_is_exact_and_goes_where_it_is_meant_to(case):
    E.check_fused_range(case, E.fused_reference(case))
    loops = E.check_fused_dispatch_and_loops(case)
    assert bool(loops) == case.loops


def test_case_names_are_unique_and_every_switch_has_a_default():
    names = [c.name for c in E.CONV_CASES + E.FUSED_CASES]
    assert len(set(names)) == len(names)
    for c in E.CONV_CASES + E.FUSED_CASES:
        assert set(dict(c.tune)) <= set(E.TUNE_DEFAULTS), c.name


def test_the_table_covers_what_it_promises():
    """Tiles per workgroup 1, 2, 3 and >= 4 with both parities in one launch on the capped persistent grid; every halo-GEMM tile
    shape per column block; XCD remap grids with q > 0 and r > 0; both weight-gradient kg values in both dtypes."""
    seen = set()
    for c in E.CONV_CASES:
        for (dt, which, per_cu), (ntiles, grid, most, fewest) in E.check_dispatch_and_loops(c).items():
            if which in ("fwd", "dx") and per_cu is None and c.tuned("FLAIR_HALO_P_WGS") == 1:
                assert most == fewest + 1
                seen.update((most, fewest))
    assert {1, 2, 3, 4} <= seen
    shapes, remap, kgs = set(), set(), set()
    for c in E.CONV_CASES:
        for dt in c.dtypes:
            fam = c.fwd_kernel(dt)[0]
            if fam.startswith("hg_"):
                tw, th, bn = E.hg_shape(c.Ho, c.Wo, c.Cout)
                nwork = c.N * c.Ho * c.Wo // (tw * th) * (c.Cout // bn)
                shapes.add((tw, th, bn))
                if nwork >= 9 and nwork % 8:
                    remap.add((tw, th, bn))
            if c.backward:
                kgs.add((dt, c.dw_kernel(dt)[0]))
    want = {(16, 8, 128), (16, 8, 64), (32, 8, 64), (16, 16, 64), (32, 8, 32), (16, 16, 32)}
    assert want <= shapes and want <= remap
    assert {(dt, k) for dt in E.DTYPES for k in ("big_kg1", "big_kg2", "halo", "plain")} <= kgs and ("bf16", "stem") in kgs


def test_gather_form_weight_gradient_splits_as_the_table_says():
    """14 splits with a short last one (both loops of the 64-wide reduce), 66 splits (the 16-wide reduce), and a gradient past the
    reduce grid's cap; one of them runs again with accumulate."""
    cases = {c.name: c for c in E.CONV_CASES}
    assert set(E.WG_PLAN_WANT) <= set(cases) and E.WG_ACCUMULATE_CASE in E.WG_PLAN_WANT
    for name in E.WG_PLAN_WANT:
        E.check_wg_plan(cases[name])
    assert {v[0] for v in E.WG_PLAN_WANT.values()} == {14, 66, 1}


def test_reduction_shapes_pass_their_caps():
    E.check_reduction_shapes()
