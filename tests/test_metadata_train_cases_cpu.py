"""tests/metadata_train_cases.py checked on the CPU, and the declaration of the two operator entry points."""
import ctypes as C
import os
import re

import torch

import metadata_train_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_integer_cases_are_exact_in_both_dtypes_and_any_order():
    for shape in tc.GRAD_SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            dx, want = tc.int_case(shape, dtype)
            assert torch.equal(dx.to(torch.float64), dx.to(torch.float64).round()) and float(dx.abs().max()) <= 8
            # fp32 sums in two very different orders give the int64 sum
            rows = dx.to(torch.float32).reshape(shape[0], shape[1], -1)
            fwd = torch.zeros(shape[:2])
            for i in range(0, rows.shape[2], 97):
                fwd = fwd + rows[:, :, i:i + 97].sum(-1)
            assert torch.equal(fwd, want) and torch.equal(rows.flip(-1).sum(-1), want)
    assert float(tc.int_case(tc.GRAD_SHAPES[-1], torch.float32)[1].abs().max()) > 0


def test_normal_case_bound_holds_for_a_sequential_fp32_sum_and_is_not_vacuous():
    dx, s64, bound = tc.normal_case((1, 2, 7, 24), torch.float32)
    seq = torch.zeros(1, 2)
    for w in range(7):
        for c in range(24):
            seq = seq + dx[:, :, w, c]
    assert bool(((seq.double() - s64).abs() <= bound).all())
    # the bound is a rounding bound: a single dropped element breaks it
    assert bool(((seq.double() - dx[:, :, 0, 0].double() - s64).abs() > bound).all())


def test_add_case_is_one_fp32_add_rounded_once():
    x, v, want = tc.add_case((2, 3, 5, 32), torch.bfloat16)
    assert want.dtype == torch.bfloat16 and not torch.equal(want, x)
    n, h, w, c = 1, 2, 4, 31
    assert want[n, h, w, c].item() == torch.tensor(x[n, h, w, c].item() + v[n, h].item(), dtype=torch.float32).to(torch.bfloat16).item()


def test_new_entry_points_are_declared_in_the_header_and_the_ctypes_table():
    from flair_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "flair_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_want in (("flair_add_rowvec_nhwc_to", 9), ("flair_rowvec_grad_nhwc", 8)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/flair_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, args = L.PROTOTYPES[name]
        assert res is L.i32 and len(args) == n_args == n_want


def test_error_texts_and_the_workspace_bound_without_a_device():
    """The dry run that sizes the arena needs no device: its result for the small executor shape is what it was before the training
    request existed (the request's extra bottleneck tensor must fit inside it — checked on the GPU)."""
    from flair_amd import _lib as L
    l = L.lib()
    assert b"drows_f32" in l.flair_strerror(-17)
    assert b"rows_f32" in l.flair_strerror(-16) and l.flair_strerror(-16) != l.flair_strerror(-17)
    for dt, name in ((0, "f32"), (1, "bf16")):
        h = C.c_void_p()
        assert l.flair_unet_create(C.byref(h), 5, 13, dt) == 0
        try:
            got = (l.flair_unet_workspace_bytes(h, 2, 160, 128, 1), l.flair_unet_workspace_bytes(h, 2, 160, 128, 0))
            assert got == tc.WORKSPACE_2x160x128[name], (name, got)
            drows = torch.full((2, 5), 7.0)     # a gradient pointer without rows: refused before anything looks behind it
            opts = L.UnetFwdOpts(drows_f32=drows.data_ptr())
            assert l.flair_unet_forward(h, None, None, None, None, 2, 160, 128, 1, None, 0, None, C.byref(opts)) == -1
            assert bool((drows == 7.0).all())
        finally:
            l.flair_unet_destroy(h)
