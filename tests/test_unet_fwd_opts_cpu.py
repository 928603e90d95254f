"""The argument structs of the C ABI against their ctypes mirrors, and the refusals of flair_unet_fwd_opts_t: flair_unet_forward
validates its options before it makes any HIP call or touches the handle, so every refusal runs without a device."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_struct(name):
    """[(field, kind)] of `typedef struct <name> { ... }` in include/flair_hip.h, in declaration order; kind is "ptr" or the
    field's integer type as the header spells it."""
    hdr = open(os.path.join(ROOT, "include", "flair_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}", hdr, flags=re.S)
    assert m, f"struct {name} is not declared in include/flair_hip.h"
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = re.fullmatch(r"((?:const )?\w+ ?\*?) ?(\w+(?: ?, ?\w+)*)", decl).groups()
        kind = "ptr" if "*" in ctype else ctype.strip()
        assert kind == "ptr" or "," not in names or "*" not in decl
        fields += [(n.strip(), kind) for n in names.split(",")]
    return fields


def _kind(ctype):
    from flair_amd import _lib as L
    return {L.vp: "ptr", L.i32: "int", L.i64: "int64_t", C.c_uint64: "uint64_t"}[ctype]


@pytest.mark.parametrize("struct,mirror", [("flair_unet_fwd_opts", "UnetFwdOpts"), ("flair_conv_ex", "ConvEx"), ("flair_wgrad_ex", "WgradEx"),
                                           ("flair_bn_bwd_ex", "BnBwdEx"), ("flair_pack_desc", "PackDesc")])
def test_ctypes_structures_mirror_the_header_field_for_field(struct, mirror):
    from flair_amd import _lib as L
    want = header_struct(struct)
    got = [(n, _kind(t)) for n, t in getattr(L, mirror)._fields_]
    assert [n for n, _ in got] == [n for n, _ in want]
    assert got == want


def test_unet_forward_takes_the_options_as_its_last_argument():
    from flair_amd import _lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flair_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+flair_unet_forward\s*\(([^;]*)\)\s*;", hdr)
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args[-1] == "const flair_unet_fwd_opts_t* opts"
    res, argtypes = L.PROTOTYPES["flair_unet_forward"]
    assert res is L.i32 and len(argtypes) == len(args) == 13 and argtypes[-1] is L.vp


# (fields, training, fp32 logits, H) -> (code, the field flair_strerror names); the table of include/flair_hip.h, in its order
_LAB, _LOSS, _WS, _PREDS, _PROB, _ROWS, _DROWS, _LOGITS = range(8)   # which stand-in buffer a field points at
_CE = dict(ce_labels=_LAB, ce_loss=_LOSS, ce_workspace=_WS)
REFUSALS = [
    # -1: the struct itself is malformed, whatever the forward
    (dict(maxprob_f32=_PROB), 0, False, 64, -1, b"maxprob_f32"),
    (dict(_CE, ce_loss=None), 0, False, 64, -1, b"ce_loss"),
    (dict(_CE, ce_workspace=None), 0, False, 64, -1, b"ce_workspace"),
    (dict(_CE, ce_label_kind=-1), 0, False, 64, -1, b"ce_label_kind"),
    (dict(_CE, ce_label_kind=4), 0, False, 64, -1, b"ce_label_kind"),
    (dict(drows_f32=_DROWS), 1, False, 64, -1, b"drows_f32"),
    (dict(drows_f32=_DROWS), 0, False, 64, -1, b"drows_f32"),
    (dict(_CE, ce_loss=None), 1, True, 48, -1, b"ce_loss"),                    # before -15 and -10
    # -15: the CE head with another head, in a training forward, with fp32 logits
    (dict(_CE, preds_u8=_PREDS), 0, False, 64, -15, b"ce_labels"),
    (dict(_CE), 1, False, 64, -15, b"ce_labels"),
    (dict(_CE), 0, True, 64, -15, b"ce_labels"),
    (dict(_CE, ce_label_kind=3), 0, True, 48, -15, b"ce_labels"),              # before -10
    (dict(_CE, rows_f32=_ROWS), 1, False, 64, -15, b"ce_labels"),              # before -16
    # -16: rows on a training forward with nowhere to put their gradient
    (dict(rows_f32=_ROWS), 1, False, 64, -16, b"rows_f32"),
    (dict(rows_f32=_ROWS), 1, True, 48, -16, b"rows_f32"),                     # before -10
    # -17: a gradient pointer on an eval-mode forward
    (dict(rows_f32=_ROWS, drows_f32=_DROWS), 0, True, 64, -17, b"drows_f32"),
    (dict(rows_f32=_ROWS, drows_f32=_DROWS), 0, False, 48, -17, b"drows_f32"),  # before -10
    # -10: the shape, with options that are fine otherwise and with none
    (dict(rows_f32=_ROWS), 0, True, 48, -10, b"divisible by 32"),
    (dict(rows_f32=_ROWS, drows_f32=_DROWS), 1, False, 48, -10, b"divisible by 32"),
    (dict(preds_u8=_PREDS, maxprob_f32=_PROB, reuse_constants=1), 0, False, 48, -10, b"divisible by 32"),
    (None, 0, True, 48, -10, b"divisible by 32"),
]


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_unet_forward_refuses_options_before_any_device_call(dt):
    """Host buffers stand in for device addresses: a refused forward reads and writes none of them."""
    from flair_amd import _lib as L
    l = L.lib()
    bufs = [torch.full((64,), 7.0) for _ in range(8)]
    pointers = {n for n, t in L.UnetFwdOpts._fields_ if t is L.vp}
    before = [b.clone() for b in bufs]
    h = C.c_void_p()
    assert l.flair_unet_create(C.byref(h), 5, 13, dt) == 0
    try:
        for fields, training, fp32_logits, H, code, names in REFUSALS:
            opts = None
            if fields is not None:
                opts = L.UnetFwdOpts(**{k: bufs[v].data_ptr() if k in pointers and v is not None else v for k, v in fields.items()})
            rc = l.flair_unet_forward(h, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                      bufs[_LOGITS].data_ptr() if fp32_logits else None, 1, H, 64, training, bufs[3].data_ptr(), 0, None,
                                      None if opts is None else C.byref(opts))
            assert rc == code, (fields, training, fp32_logits, H, rc)
            assert names in l.flair_strerror(rc), (rc, l.flair_strerror(rc))
        assert l.flair_unet_forward(None, None, None, None, None, 1, 64, 64, 0, None, 0, None, None) == -1
    finally:
        l.flair_unet_destroy(h)
    assert all(torch.equal(a, b) for a, b in zip(bufs, before))
