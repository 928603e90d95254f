"""The case table of flair_add_rowvec_nhwc (tests/metadata_eval_cases.py) checked on the CPU: the planted bf16 ties, the expectations
against a naive NCHW loop with a rounding of its own, and the declaration of the operator's entry point."""
import os
import re

import numpy as np
import torch

import metadata_eval_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bf16_rne(f):
    """fp32 scalar -> nearest bf16 (ties to even) as fp32, on the bit pattern."""
    u = int(np.float32(f).view(np.uint32))
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return np.uint32(u).view(np.float32)


def _naive_nchw(x_nhwc, v, bf16):
    """out[n][c][h][w] = x[n][c][h][w] + v[n][h], one fp32 add per element (model.py:59-60 read literally), as NHWC."""
    x = x_nhwc.float().permute(0, 3, 1, 2).contiguous().numpy()
    vv = v.numpy()
    out = np.empty_like(x)
    Nn, Cc, Hh, Ww = x.shape
    for n in range(Nn):
        for c in range(Cc):
            for h in range(Hh):
                for w in range(Ww):
                    s = np.float32(x[n, c, h, w]) + np.float32(vv[n, h])
                    out[n, c, h, w] = _bf16_rne(s) if bf16 else s
    return torch.from_numpy(out).permute(0, 2, 3, 1).contiguous()


def test_planted_ties_round_as_stated():
    x, v, want = mc.case(torch.bfloat16)
    for (n, h, w, c), xv, vv, res in mc.TIES:
        assert x[n, h, w, c].item() == xv and v[n, h].item() == vv      # representable as planted
        assert want[n, h, w, c].item() == res, ((n, h, w, c), want[n, h, w, c].item(), res)
    # the four as the issue lists them
    got = [want[idx].item() for idx, _, _, _ in mc.TIES]
    assert got == [1.0, 1.0 + 2.0 ** -6, 3.015625, -1.0]
    # in fp32 the same sums are exact
    xf, vf, wf = mc.case(torch.float32)
    for (n, h, w, c), xv, vv, _ in mc.TIES:
        assert wf[n, h, w, c].item() == np.float32(xv) + np.float32(vv)


def test_expectations_equal_a_naive_nchw_loop():
    for dtype in (torch.float32, torch.bfloat16):
        x, v, want = mc.case(dtype)
        assert tuple(x.shape) == (3, 5, 2, 24) and tuple(v.shape) == (3, 5) and want.dtype == dtype
        naive = _naive_nchw(x, v, dtype == torch.bfloat16)
        assert torch.equal(want.float(), naive)
        assert not torch.equal(want, x)


def test_new_entry_points_are_declared_in_the_header_and_the_ctypes_table():
    """(the forward's rows_f32 option: the struct-mirror test of test_unet_fwd_opts_cpu.py)"""
    from flair_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "flair_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_want in (("flair_add_rowvec_nhwc", 8),):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/flair_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        res, args = L.PROTOTYPES[name]
        assert res is L.i32 and len(args) == n_args == n_want
