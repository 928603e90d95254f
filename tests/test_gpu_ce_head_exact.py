"""Operator tests of the cross-entropy head (csrc/ce_head.hip) against torch's fp64 cross entropy: flair_ce_head_nhwc in its six
instantiations (row stride 16 / 24 / 32 x fp32 / bf16), flair_ce_head with its four-pixel and one-pixel kernels writing NCHW and
NHWC gradients, both softmax-argmax entries, flair_confmat_update and flair_jaccard.  tests/ce_head_cases.py has the cases, the
references and the bounds; test_ce_head_cases_cpu.py shows that an fp32 restatement of the kernels' arithmetic keeps those bounds
with 4x to spare and that fp32 and fp64 argmax agree on every pixel, so predictions and confusion matrices are compared for
equality.

Every output sits inside a larger allocation whose surroundings must come back untouched: 64 rows before and after the gradient
rows (prefilled with NaN), sentinel bytes around predictions, targets, the confusion matrix and the loss, and a workspace of exactly
flair_ce_workspace_bytes.  The NHWC logits lie in an allocation long enough for a 32-column walk over the rows, its padded columns
and its tail holding 250: a kernel that walks the wrong stride or looks at a padded column computes something else and fails.

Nothing here needs more than one process or 200 MB of device memory; the file takes well under a minute on an MI355X."""
import numpy as np
import pytest
import torch

import ce_head_cases as K

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
KIND_CODE = {"u8": 0, "i32": 1, "i64": 2, "onehot": 3}
GUARD_ROWS = 64
GUARD = 256              # elements around the flat outputs
JUNK = 250.0             # in padded logit columns and behind the rows: a bf16 number above every logit
CM_FILL = 2 ** 40


def _bits(t):
    """The tensor as integers of its element size: NaN compares equal to itself, -0.0 differs from +0.0."""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class _Guarded:
    """n elements of `dtype` inside an allocation of n + 2 * guard (+ off) elements filled with `fill`; ptr is the region's address."""

    def __init__(self, dev, n, dtype, fill, guard=GUARD, off=0):
        self.n, self.lo = n, guard + off
        self.full = torch.full((n + 2 * guard + off,), fill, dtype=dtype, device=dev)
        self.before = _bits(self.full.cpu().clone())
        self.ptr = self.full.data_ptr() + self.lo * self.full.element_size()

    def read(self, what):
        """The region on the host, after checking that nothing outside it changed."""
        after = self.full.cpu()
        a = _bits(after)
        assert torch.equal(a[:self.lo], self.before[:self.lo]), f"{what}: written before the buffer"
        assert torch.equal(a[self.lo + self.n:], self.before[self.lo + self.n:]), f"{what}: written behind the buffer"
        return after[self.lo:self.lo + self.n]


def _labels(v, kind, dev):
    return v["lab"][kind].to(dev).contiguous()


def _outputs(dev, npix, C, ld, dl_dtype, preds_off=0):
    return {
        "dl": _Guarded(dev, npix * ld, dl_dtype, float("nan"), guard=GUARD_ROWS * ld) if ld else None,
        "preds": _Guarded(dev, npix, torch.uint8, 0xA5, off=preds_off),
        "targets": _Guarded(dev, npix, torch.int32, 0x5A5A5A5A),
        "cm": _Guarded(dev, C * C, torch.int64, -7, guard=8),
        "loss": _Guarded(dev, 1, torch.float32, 7.0, guard=4),
    }


def _lib():
    from flair_amd import _lib as L
    return L


def _workspace(dev, shape):
    L = _lib()
    n = L.lib().flair_ce_workspace_bytes(*shape)
    assert n % 4 == 0
    return _Guarded(dev, n, torch.uint8, 0xC3)


def _collect(o, ws, npix, C, ld, what):
    torch.cuda.synchronize()
    ws.read(what + " workspace")
    r = {"loss": float(o["loss"].read(what + " loss")[0]),
         "preds": o["preds"].read(what + " preds"),
         "targets": o["targets"].read(what + " targets"),
         "cm": o["cm"].read(what + " confmat").view(C, C) - CM_FILL}
    if o["dl"] is not None:
        r["dl"] = o["dl"].read(what + " dlogits_nhwc").view(npix, ld)
    return r


def _fill_cm(o):
    o["cm"].full[o["cm"].lo:o["cm"].lo + o["cm"].n] = CM_FILL


def run_nhwc(dev, C, ld, shape, x, labels, kind, w, dt, want_dl=True):
    """flair_ce_head_nhwc on guarded buffers -> dict loss, preds (npix,) u8, targets (npix,) i32, cm (C, C) counted, dl (npix, ld)."""
    L = _lib()
    npix = shape[0] * shape[1] * shape[2]
    rows = K.nhwc_rows(x, ld, fill=JUNK)
    walk = (npix * 32 + ld - 1) // ld + GUARD_ROWS          # rows a 32-column walk would touch, and some
    buf = torch.full((walk, ld), JUNK)
    buf[:npix] = rows
    buf = buf.to(device=dev, dtype=TDT[dt])
    o = _outputs(dev, npix, C, ld, TDT[dt])
    _fill_cm(o)
    ws = _workspace(dev, shape)
    wd = None if w is None else w.to(dev)
    rc = L.lib().flair_ce_head_nhwc(buf.data_ptr(), L.dtype_code(TDT[dt]), ld, L.ptr(labels), KIND_CODE[kind], L.ptr(wd),
                                    shape[0], C, shape[1], shape[2], o["loss"].ptr, o["dl"].ptr if want_dl else None,
                                    o["preds"].ptr, o["targets"].ptr, o["cm"].ptr, ws.ptr, L.stream())
    assert rc == 0, rc
    r = _collect(o, ws, npix, C, ld, f"nhwc {dt} ld{ld}")
    assert torch.equal(_bits(buf.cpu()[npix:]), _bits(torch.full((walk - npix, ld), JUNK, dtype=TDT[dt]))), "the logits were written"
    return r


def run_nchw(dev, C, shape, x, labels, kind, w, dl_ld=0, dl_dt="f32", want_dl=True, misalign=""):
    """flair_ce_head on guarded buffers; misalign: the pointer that sits one element off its natural place.  Adds dl_nchw (B, C, H, W)."""
    L = _lib()
    B, H, W = shape
    npix = B * H * W
    xin = _Guarded(dev, x.numel(), torch.float32, JUNK, off=1 if misalign == "logits" else 0)
    xin.full[xin.lo:xin.lo + xin.n] = x.reshape(-1).to(dev)
    o = _outputs(dev, npix, C, dl_ld, TDT[dl_dt], preds_off=1 if misalign == "preds" else 0)
    _fill_cm(o)
    dn = _Guarded(dev, x.numel(), torch.float32, float("nan"), off=1 if misalign == "dlogits" else 0) if want_dl else None
    if misalign:
        p = {"logits": xin.ptr, "preds": o["preds"].ptr, "dlogits": dn.ptr if dn else 16}[misalign]
        assert p % 16 != 0 and (misalign != "preds" or p % 4 != 0)
    else:
        assert xin.ptr % 16 == 0 and o["preds"].ptr % 4 == 0 and (dn is None or dn.ptr % 16 == 0)
    ws = _workspace(dev, shape)
    wd = None if w is None else w.to(dev)
    rc = L.lib().flair_ce_head(xin.ptr, L.ptr(labels), KIND_CODE[kind], L.ptr(wd), B, C, H, W, o["loss"].ptr,
                               dn.ptr if dn else None, o["dl"].ptr if dl_ld else None, L.dtype_code(TDT[dl_dt]), dl_ld,
                               o["preds"].ptr, None, o["targets"].ptr, o["cm"].ptr, ws.ptr, L.stream())
    assert rc == 0, rc
    r = _collect(o, ws, npix, C, dl_ld, f"nchw dl_ld{dl_ld} {dl_dt}")
    xin.read("logits")
    if dn is not None:
        r["dl_nchw"] = dn.read("dlogits_nchw").view(B, C, H, W)
    return r


def _rows_of(dl_nchw):
    B, C, H, W = dl_nchw.shape
    return dl_nchw.permute(0, 2, 3, 1).reshape(-1, C)


def check_rows(dl, C, valid, what):
    """Item 2: columns C.. of every row are +0.0 bit for bit, rows of ignored pixels hold zeros, nothing is left of the NaN prefill
    (where some pixel counts)."""
    if dl.shape[1] > C:
        assert int(_bits(dl[:, C:]).ne(0).sum()) == 0, f"{what}: padded columns are not +0.0"
    ign = ~valid.reshape(-1)
    if ign.any():
        assert float(dl[ign].float().abs().max()) == 0.0, f"{what}: an ignored pixel has a gradient"
    assert bool(torch.isfinite(dl.float()).all()), f"{what}: NaN or inf in the gradient rows"


def check_against_reference(r, ref, v, kind, C, what):
    """Item 1: predictions, confusion matrix and targets equal the reference; the loss within its bound."""
    lab = v["lab"]
    assert torch.equal(r["preds"].long(), ref["preds"].reshape(-1)), f"{what}: preds"
    assert np.array_equal(r["cm"].numpy(), ref["confmat"]), f"{what}: confusion matrix"
    tg = r["targets"].long()
    if kind == "onehot":
        assert torch.equal(tg, lab["y_onehot"].reshape(-1)), f"{what}: targets"
    else:
        exact, fits = K.expected_targets(lab[kind].reshape(-1), C)
        assert torch.equal(tg[fits], exact[fits]), f"{what}: targets where int32 holds the label"
        assert bool(((tg[~fits] < 0) | (tg[~fits] >= C)).all()), f"{what}: a wide ignored label became a class"
    err, bound = abs(r["loss"] - ref["loss"]), K.loss_bound(ref["loss"])
    print(f"{what}: loss {r['loss']:.9f} fp64 {ref['loss']:.9f} err {err:.2e} (bound {bound:.2e})")
    assert np.isfinite(r["loss"]) and err <= bound, (what, r["loss"], ref["loss"])


def check_dl_f32(dl, ref_dl, C, what):
    err = float((dl[:, :C].double() - _rows_of(ref_dl)).abs().max())
    bound = K.dl_bound(ref_dl)
    print(f"{what}: max |dl - fp64| {err:.2e} (bound {bound:.2e})")
    assert err <= bound, (what, err, bound)


def _valid(v, kind):
    return torch.ones_like(v["lab"]["ign"]) if kind == "onehot" else ~v["lab"]["ign"]


def _kinds(case):
    """Label kinds a case runs with: all four at the small shapes; the two large cases share them out."""
    if case.shape != K.LARGE:
        return K.KINDS
    return ("i64", "onehot") if case.ld == 16 else ("u8", "i32")


# ------------------------------------------------------------------------------------------------ 1, 2: the NHWC head
@pytest.mark.parametrize("case", K.NHWC_CASES, ids=lambda c: c.name)
def test_nhwc_head_against_fp64_cross_entropy(dev, case):
    """Both dtypes of every case, every label kind.  fp32: loss and gradient inside the project's bounds of the fp64 reference.
    bf16: the gradient is bit for bit the round-to-nearest-even bf16 of what the fp32 instantiation wrote for the same values (the
    two differ only in load and store); its loss, predictions and counts are the fp32 instantiation's own."""
    v = K.case_values(*case.values)
    C, ld = case.C, case.ld
    for kind in _kinds(case):
        ref = v["onehot" if kind == "onehot" else "int"]
        labels = _labels(v, kind, dev)
        got = {}
        for dt in K.DTYPES:
            what = f"{case.name} {kind} {case.kernel(dt)}"
            r = got[dt] = run_nhwc(dev, C, ld, case.shape, v["x"], labels, kind, v["w"], dt)
            check_against_reference(r, ref, v, kind, C, what)
            check_rows(r["dl"], C, _valid(v, kind), what)
        check_dl_f32(got["f32"]["dl"], ref["dl"], C, f"{case.name} {kind} f32")
        want = got["f32"]["dl"].to(torch.bfloat16)      # torch rounds to nearest even
        assert torch.equal(_bits(got["bf16"]["dl"]), _bits(want)), f"{case.name} {kind}: bf16 rows are not RNE(fp32 rows)"
        assert got["bf16"]["loss"] == got["f32"]["loss"], (got["bf16"]["loss"], got["f32"]["loss"])


@pytest.mark.parametrize("dt", K.DTYPES)
@pytest.mark.parametrize("C,ld", K.C_LD)
def test_nhwc_head_without_a_gradient_leaves_the_rest_alone(dev, C, ld, dt):
    """dlogits_nhwc = NULL: loss, predictions and counts are those of the call with a gradient, and no row is written (the guarded
    gradient buffer is handed to nobody and comes back as it was)."""
    case = next(c for c in K.NHWC_CASES if (c.C, c.ld, c.shape) == (C, ld, K.SMALL))
    v = K.case_values(*case.values)
    labels = _labels(v, "i32", dev)
    a = run_nhwc(dev, C, ld, case.shape, v["x"], labels, "i32", v["w"], dt)
    b = run_nhwc(dev, C, ld, case.shape, v["x"], labels, "i32", v["w"], dt, want_dl=False)
    assert a["loss"] == b["loss"] and torch.equal(a["preds"], b["preds"]) and torch.equal(a["cm"], b["cm"])
    assert bool(torch.isnan(b["dl"].float()).all())


# ------------------------------------------------------------------------------------------------ 3, 4, 5: the NCHW entry
ALIGNED_NCHW = [c for c in K.NCHW_CASES if not c.misalign]


@pytest.mark.parametrize("case", ALIGNED_NCHW, ids=lambda c: c.name)
def test_nchw_entry_against_fp64_and_its_nhwc_rows(dev, case):
    """flair_ce_head against the reference, and what it writes through dlogits_nhwc: fp32 rows are the NCHW gradient permuted,
    bit for bit, bf16 rows its round-to-nearest-even; the same rows come out when no NCHW gradient is asked for.  Cases are
    chosen so that both the four-pixel and the one-pixel kernel write rows of 16, 24 and 32 columns (ce_head_cases.nchw_kernel)."""
    v = K.case_values(*case.values)
    C = case.C
    for kind in ("u8", "i64") if case.dl_ld else K.KINDS:
        ref = v["onehot" if kind == "onehot" else "int"]
        labels = _labels(v, kind, dev)
        base = run_nchw(dev, C, case.shape, v["x"], labels, kind, v["w"])
        what = f"{case.name} {kind} {case.kernel}"
        check_against_reference(base, ref, v, kind, C, what)
        rows = _rows_of(base["dl_nchw"])
        check_dl_f32(rows, ref["dl"], C, what)
        assert bool(torch.isfinite(rows).all())
        if not case.dl_ld:
            continue
        for dl_dt in K.DTYPES:
            want = torch.zeros(case.npix, case.dl_ld)
            want[:, :C] = rows
            want = want.to(TDT[dl_dt])
            for want_dl in (True, False):
                r = run_nchw(dev, C, case.shape, v["x"], labels, kind, v["w"], case.dl_ld, dl_dt, want_dl=want_dl)
                w2 = f"{what} rows {dl_dt} ld{case.dl_ld} nchw gradient {'on' if want_dl else 'off'}"
                check_rows(r["dl"], C, _valid(v, kind), w2)
                # (value -0.0 where a weight of zero meets p - 1: the bits say so on both sides)
                assert torch.equal(_bits(r["dl"]), _bits(want)), w2
                assert torch.equal(r["preds"], base["preds"]) and torch.equal(r["cm"], base["cm"]) and torch.equal(r["targets"], base["targets"])
                if want_dl:
                    assert torch.equal(_bits(r["dl_nchw"]), _bits(base["dl_nchw"])), w2
                # with rows wider than its register row the entry takes the one-pixel kernel: another summation order
                assert abs(r["loss"] - base["loss"]) <= K.loss_bound(ref["loss"])
                if K.nchw_kernel(C, case.shape, case.dl_ld, False) == K.nchw_kernel(C, case.shape, 0, False):
                    assert r["loss"] == base["loss"]


@pytest.mark.parametrize("case", [c for c in ALIGNED_NCHW if c.dl_ld], ids=lambda c: c.name)
def test_layouts_agree(dev, case):
    """The same values through flair_ce_head and flair_ce_head_nhwc (fp32 and bf16 rows): identical predictions, confusion
    matrix and fp32 gradient bits.  The one-pixel NCHW kernel and the NHWC kernel map one pixel to one thread on the same grid:
    their losses are bit-identical; the four-pixel kernel sums its partials in another order and stays within the loss bound."""
    v = K.case_values(*case.values)
    C, ld = case.C, case.dl_ld
    labels = _labels(v, "i32", dev)
    ref = v["int"]
    a = run_nchw(dev, C, case.shape, v["x"], labels, "i32", v["w"], ld, "f32")
    for dt in K.DTYPES:
        b = run_nhwc(dev, C, ld, case.shape, v["x"], labels, "i32", v["w"], dt)
        assert torch.equal(a["preds"], b["preds"]) and torch.equal(a["cm"], b["cm"]) and torch.equal(a["targets"], b["targets"])
        if dt == "f32":
            assert torch.equal(_bits(a["dl"]), _bits(b["dl"])), "NHWC rows of the two entries"
            assert torch.equal(_bits(_rows_of(a["dl_nchw"])), _bits(b["dl"][:, :C])), "NCHW gradient against NHWC rows"
        print(f"{case.name} {case.kernel} vs nhwc {dt}: loss {a['loss']:.9f} / {b['loss']:.9f}")
        if case.kernel.startswith("scalar"):
            assert a["loss"] == b["loss"], (a["loss"], b["loss"])
        else:
            assert abs(a["loss"] - b["loss"]) <= K.loss_bound(ref["loss"])
            assert abs(b["loss"] - ref["loss"]) <= K.loss_bound(ref["loss"])


@pytest.mark.parametrize("case", [c for c in K.NCHW_CASES if c.misalign], ids=lambda c: c.name)
def test_a_pointer_off_its_alignment_takes_the_one_pixel_kernel_to_the_same_result(dev, case):
    """H*W % 4 == 0 and logits one float, predictions one byte or the NCHW gradient one float off: the entry must not use 16-byte
    accesses.  Predictions, confusion matrix and gradient are bit-equal to the aligned call's, the loss within the bound."""
    v = K.case_values(*case.values)
    C = case.C
    assert (case.shape[1] * case.shape[2]) % 4 == 0
    labels = _labels(v, "i64", dev)
    ref = v["int"]
    a = run_nchw(dev, C, case.shape, v["x"], labels, "i64", v["w"], case.dl_ld, "f32")
    b = run_nchw(dev, C, case.shape, v["x"], labels, "i64", v["w"], case.dl_ld, "f32", misalign=case.misalign)
    assert torch.equal(a["preds"], b["preds"]) and torch.equal(a["cm"], b["cm"]) and torch.equal(a["targets"], b["targets"])
    assert torch.equal(_bits(a["dl_nchw"]), _bits(b["dl_nchw"]))
    if case.dl_ld:
        assert torch.equal(_bits(a["dl"]), _bits(b["dl"]))
    check_against_reference(b, ref, v, "i64", C, case.name)
    assert abs(a["loss"] - b["loss"]) <= K.loss_bound(ref["loss"])


def _softmax_nchw(dev, x, off_logits=0, off_preds=0, off_maxprob=0):
    L = _lib()
    B, C, H, W = x.shape
    npix = B * H * W
    xin = _Guarded(dev, x.numel(), torch.float32, JUNK, off=off_logits)
    xin.full[xin.lo:xin.lo + xin.n] = x.reshape(-1).to(dev)
    pu8 = _Guarded(dev, npix, torch.uint8, 0xA5, off=off_preds)
    pi64 = _Guarded(dev, npix, torch.int64, -7)
    mp = _Guarded(dev, npix, torch.float32, float("nan"), off=off_maxprob)
    assert (xin.ptr % 16 == 0) == (off_logits == 0) and (pu8.ptr % 4 == 0) == (off_preds == 0) and (mp.ptr % 16 == 0) == (off_maxprob == 0)
    assert L.lib().flair_softmax_argmax(xin.ptr, B, C, H, W, pu8.ptr, pi64.ptr, mp.ptr, L.stream()) == 0
    torch.cuda.synchronize()
    return pu8.read("preds_u8"), pi64.read("preds_i64"), mp.read("maxprob")


def _softmax_nhwc(dev, x, ld, dt):
    L = _lib()
    B, C, H, W = x.shape
    npix = B * H * W
    walk = (npix * 32 + ld - 1) // ld + GUARD_ROWS
    buf = torch.full((walk, ld), JUNK)
    buf[:npix] = K.nhwc_rows(x, ld, fill=JUNK)
    buf = buf.to(device=dev, dtype=TDT[dt])
    pu8 = _Guarded(dev, npix, torch.uint8, 0xA5)
    pi64 = _Guarded(dev, npix, torch.int64, -7)
    mp = _Guarded(dev, npix, torch.float32, float("nan"))
    assert L.lib().flair_softmax_argmax_nhwc(buf.data_ptr(), L.dtype_code(TDT[dt]), ld, B, C, H, W, pu8.ptr, pi64.ptr, mp.ptr, L.stream()) == 0
    torch.cuda.synchronize()
    return pu8.read("preds_u8"), pi64.read("preds_i64"), mp.read("maxprob")


@pytest.mark.parametrize("family", ["ints", "far"])
@pytest.mark.parametrize("C", [13, 19])
def test_softmax_argmax_routing_by_alignment_and_far_logits(dev, C, family):
    """flair_softmax_argmax, aligned (the four-pixel kernel) and with logits, predictions or maxprob one element off (the
    one-pixel kernel with H*W % 4 == 0): the same bits.  Both entries on the far family: predictions equal fp64's, maxprob
    within the existing 1e-6."""
    v = K.case_values(C, K.MEDIUM, family, "rand")
    ref = v["int"]
    pu8, pi64, mp = _softmax_nchw(dev, v["x"])
    assert torch.equal(pi64, ref["preds"].reshape(-1)) and torch.equal(pu8.long(), pi64)
    err = float((mp.double() - ref["maxprob"].reshape(-1)).abs().max())
    print(f"softmax_argmax C={C} {family}: max |maxprob - fp64| {err:.2e}")
    assert err <= K.MAXPROB_ATOL
    for off in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        assert not K.softmax_routes_vec4(K.MEDIUM[1] * K.MEDIUM[2], False)
        q8, q64, mq = _softmax_nchw(dev, v["x"], *off)
        assert torch.equal(q8, pu8) and torch.equal(q64, pi64) and torch.equal(_bits(mq), _bits(mp)), off
    ld = 16 if C <= 16 else 32
    for dt in K.DTYPES:
        q8, q64, mq = _softmax_nhwc(dev, v["x"], ld, dt)
        assert torch.equal(q64, ref["preds"].reshape(-1)) and torch.equal(q8.long(), q64)
        assert float((mq.double() - ref["maxprob"].reshape(-1)).abs().max()) <= K.MAXPROB_ATOL
        assert torch.equal(_bits(mq), _bits(mp)), "the layouts run the same arithmetic"


def test_far_logits_stay_finite_through_every_loss_entry(dev):
    """Logits at +-120: a pixel's loss term is near 100 and exp(x - max) underflows for most classes.  Loss and gradient are
    finite and inside the bounds through flair_ce_head (both kernels) and flair_ce_head_nhwc (both dtypes)."""
    v = K.case_values(19, K.MEDIUM, "far", "rand")
    ref, labels = v["int"], _labels(v, "u8", dev)
    assert ref["loss"] > 40
    runs = {"nchw four-pixel": run_nchw(dev, 19, K.MEDIUM, v["x"], labels, "u8", v["w"]),
            "nchw one-pixel": run_nchw(dev, 19, K.MEDIUM, v["x"], labels, "u8", v["w"], misalign="logits"),
            "nhwc f32 ld24": run_nhwc(dev, 19, 24, K.MEDIUM, v["x"], labels, "u8", v["w"], "f32"),
            "nhwc f32 ld32": run_nhwc(dev, 19, 32, K.MEDIUM, v["x"], labels, "u8", v["w"], "f32")}
    for what, r in runs.items():
        check_against_reference(r, ref, v, "u8", 19, "far " + what)
        dl = _rows_of(r["dl_nchw"]) if "dl_nchw" in r else r["dl"]
        assert bool(torch.isfinite(dl).all())
        check_dl_f32(dl, ref["dl"], 19, "far " + what)
    b = run_nhwc(dev, 19, 32, K.MEDIUM, v["x"], labels, "u8", v["w"], "bf16")
    assert b["loss"] == runs["nhwc f32 ld32"]["loss"] and bool(torch.isfinite(b["dl"].float()).all())


# ------------------------------------------------------------------------------------------------ 7: nothing valid
@pytest.mark.parametrize("how", ["all_ignored_u8", "all_ignored_i64_wide", "present_classes_weigh_nothing"])
def test_nothing_valid(dev, how):
    """No pixel carries weight: the loss is 0 / 0 = NaN, as torch's is; predictions equal the reference; buffers around the
    outputs stay intact.  With every label ignored the confusion matrix is unchanged; where the labels are valid and only their
    weights are zero it counts them, as the reference's does (torchmetrics knows no weights).

    The gradient's values are not asserted.  torch gives 0 where every label is ignored and NaN where the weights are zero; the
    kernels form w * (1 / den) = 0 * inf in both and write NaN into the C columns of every row (padded columns stay +0.0),
    measured on an MI355X, through both entries and in both dtypes."""
    C, ld, shape = 13, 16, K.SMALL
    v = K.case_values(C, shape, "ints", "rand")
    lab = v["lab"]
    if how == "all_ignored_u8":
        labels, kind, w, valid = torch.full(shape, 255, dtype=torch.uint8), "u8", v["w"], torch.zeros(shape, dtype=torch.bool)
    elif how == "all_ignored_i64_wide":     # every one of these narrows to a class with (int)
        labels, kind, w, valid = lab["y"] + 2 ** 32, "i64", v["w"], torch.zeros(shape, dtype=torch.bool)
    else:
        w = torch.zeros(C)
        w[K.ABSENT_CLASS] = 1.0
        labels, kind, valid = lab["y"].to(torch.int32), "i32", torch.ones(shape, dtype=torch.bool)
    ref = K.reference_of(v["x"], lab["y"], valid, w)
    assert np.isnan(ref["loss"])
    for entry in ("nhwc_f32", "nhwc_bf16", "nchw"):
        if entry == "nchw":
            r = run_nchw(dev, C, shape, v["x"], labels.to(dev), kind, w, ld, "f32")
        else:
            r = run_nhwc(dev, C, ld, shape, v["x"], labels.to(dev), kind, w, entry[5:])
        assert np.isnan(r["loss"]), (how, entry, r["loss"])
        assert torch.equal(r["preds"].long(), ref["preds"].reshape(-1))
        assert np.array_equal(r["cm"].numpy(), ref["confmat"])
        if not valid.any():
            assert int(r["cm"].abs().sum()) == 0
        dl = r["dl"].float()
        print(f"{how} {entry}: gradient NaN in {int(torch.isnan(dl[:, :C]).sum())} of {dl[:, :C].numel()} class columns, "
              f"torch: NaN in {int(torch.isnan(ref['dl']).sum())}, zeros in {int((ref['dl'] == 0).sum())}")
        assert int(_bits(r["dl"][:, C:]).ne(0).sum()) == 0


# ------------------------------------------------------------------------------------------------ 8: Jaccard and confmat_update
@pytest.mark.parametrize("name", sorted(K.jaccard_matrices()))
def test_jaccard_edges(dev, name):
    """flair_jaccard against seg_step.jaccard_from_confmat.  Sums of int64 counts up to 32 * 2^41 are exact in fp64 on both sides
    and a class's quotient is one fp64 division of the same two numbers: per class the result is the fp32 rounding of the
    oracle's.  The two averages add the same fp64 terms in another order (a relative difference of a few 2^-53) before they are
    rounded to fp32: at most one fp32 ulp between them."""
    from flair_amd import ops
    from oracle import seg_step
    cm = K.jaccard_matrices()[name]
    per, wt, mac = ops.jaccard(cm.to(dev))
    ref = seg_step.jaccard_from_confmat(cm.numpy(), None)
    assert np.array_equal(per.cpu().numpy(), ref.astype(np.float32)), (per.cpu().numpy(), ref)
    for got, avg in ((wt, "weighted"), (mac, "macro")):
        want = float(seg_step.jaccard_from_confmat(cm.numpy(), avg))
        assert abs(float(got) - want) <= 2.0 ** -23 * abs(want), (name, avg, float(got), want)
        assert want != 0 or float(got) == 0


@pytest.mark.parametrize("C", [1, 13, 32])
def test_confmat_update_drops_wide_out_of_range_members(dev, C):
    """int64 targets and predictions with values that an (int) cast folds into [0, C) - 2^32 + 3, -(2^32) + 1, 2^32 - must be
    dropped like any other out-of-range member; int32 and uint8 members with their own out-of-range values as well.  The matrix
    is prefilled with 2^40 per cell."""
    from flair_amd import ops
    from oracle import seg_step
    g = torch.Generator().manual_seed(C)
    n = 4099
    wide = torch.tensor(list(K.IGNORED_I64[:1] + K.IGNORED_I64[2:]) + [C, 2 ** 32, 2 ** 32 + C - 1, -(2 ** 32), 2 ** 33 + 0])
    t = torch.randint(0, C, (n,), generator=g)
    p = torch.randint(0, C, (n,), generator=g)
    it = torch.randperm(n, generator=g)[:600]
    t[it] = wide[torch.arange(600) % len(wide)]
    ip = torch.randperm(n, generator=g)[:300]
    p[ip] = wide[(torch.arange(300) + 3) % len(wide)]
    want = seg_step.confusion_matrix_np(t.numpy(), p.numpy(), C)
    assert want.sum() < n - 500
    cm = ops.confmat_update(torch.full((C, C), CM_FILL, dtype=torch.int64, device=dev), t.to(dev), p.to(dev))
    assert np.array_equal(cm.cpu().numpy() - CM_FILL, want)
    # narrower kinds: int32 targets with -1 / C / 255 / 2^31 - 1, uint8 predictions with 255 and C
    t32 = torch.randint(0, C, (n,), generator=g)
    t32[it] = torch.tensor([C if x is None else x for x in K.IGNORED_I32])[torch.arange(600) % 4]
    p8 = torch.randint(0, C, (n,), generator=g)
    p8[ip] = torch.tensor([255, C])[torch.arange(300) % 2]
    want = seg_step.confusion_matrix_np(t32.numpy(), p8.numpy(), C)
    cm = ops.confmat_update(torch.full((C, C), CM_FILL, dtype=torch.int64, device=dev), t32.to(torch.int32).to(dev), p8.to(torch.uint8).to(dev))
    assert np.array_equal(cm.cpu().numpy() - CM_FILL, want)


# ------------------------------------------------------------------------------------------------ 9: refusals
def test_refusals_come_before_any_launch(dev):
    """Return codes of the calls the head refuses; every output buffer and the workspace come back as they were filled, so nothing
    ran.  -1: a required pointer is null or the label kind unknown; -2: channel count or dtype; -3: row stride, or (new) NHWC
    logits / gradient rows off 16 bytes, workspace off 4 bytes."""
    L = _lib()
    l = L.lib()
    C, ld, shape = 13, 16, K.SMALL
    B, H, W = shape
    npix = B * H * W
    x = torch.zeros(npix + 8, 32, device=dev)
    xb = x.to(torch.bfloat16)
    lab = torch.zeros(shape, dtype=torch.uint8, device=dev)
    o = _outputs(dev, npix, 32, 32, torch.float32)
    ws = _workspace(dev, shape)
    s = L.stream()

    def nhwc(logits=x.data_ptr(), dtype=0, ld=ld, labels=lab.data_ptr(), kind=0, C=C, loss=o["loss"].ptr, dl=o["dl"].ptr, wsp=ws.ptr):
        return l.flair_ce_head_nhwc(logits, dtype, ld, labels, kind, None, B, C, H, W, loss, dl, o["preds"].ptr, o["targets"].ptr,
                                    o["cm"].ptr, wsp, s)

    def nchw(logits=x.data_ptr(), labels=lab.data_ptr(), kind=0, C=C, loss=o["loss"].ptr, dl=o["dl"].ptr, dl_dt=0, dl_ld=ld, wsp=ws.ptr):
        return l.flair_ce_head(logits, labels, kind, None, B, C, H, W, loss, None, dl, dl_dt, dl_ld, o["preds"].ptr, None,
                               o["targets"].ptr, o["cm"].ptr, wsp, s)

    for bad in (8, 12, 20, 28, 40, 0):
        assert nhwc(ld=bad) == -3, bad
    assert nhwc(C=17, ld=16) == -3 and nhwc(C=25, ld=24) == -3
    assert nhwc(C=0) == -2 and nhwc(C=33, ld=32) == -2
    assert nhwc(dtype=2) == -2 and nhwc(dtype=-1) == -2
    assert nhwc(kind=-1) == -1 and nhwc(kind=4) == -1
    assert nhwc(logits=None) == -1 and nhwc(labels=None) == -1 and nhwc(loss=None) == -1 and nhwc(wsp=None) == -1
    # (new) every NHWC row is read and written in 16-byte chunks; the workspace holds fp32 partial sums
    assert nhwc(logits=x.data_ptr() + 4) == -3 and nhwc(logits=x.data_ptr() + 8) == -3
    assert nhwc(logits=xb.data_ptr() + 2, dtype=1) == -3 and nhwc(logits=xb.data_ptr() + 8, dtype=1) == -3
    assert nhwc(dl=o["dl"].ptr + 4) == -3 and nhwc(dtype=1, logits=xb.data_ptr(), dl=o["dl"].ptr + 2) == -3
    assert nhwc(wsp=ws.ptr + 1) == -3 and nhwc(wsp=ws.ptr + 2) == -3
    assert nchw(dl_ld=12) == -3                       # < C
    assert nchw(dl_ld=36) == -3 and nchw(dl_ld=40) == -3
    assert nchw(dl_ld=18) == -3 and nchw(dl_ld=14) == -3       # fp32 rows: whole 16-byte chunks are multiples of 4
    assert nchw(dl_ld=20, dl_dt=1) == -3 and nchw(dl_ld=28, dl_dt=1) == -3     # bf16: multiples of 8
    assert nchw(dl=o["dl"].ptr + 4) == -3 and nchw(dl=o["dl"].ptr + 8, dl_dt=1) == -3
    assert nchw(wsp=ws.ptr + 2) == -3
    assert nchw(C=0) == -2 and nchw(C=33) == -2
    assert nchw(kind=-1) == -1 and nchw(kind=4) == -1
    assert nchw(logits=None) == -1 and nchw(labels=None) == -1 and nchw(loss=None) == -1 and nchw(wsp=None) == -1
    # the loss head takes rows of 24 columns, the predict entry does not: pinned as it is
    pu8 = _Guarded(dev, npix, torch.uint8, 0xA5)
    assert l.flair_softmax_argmax_nhwc(x.data_ptr(), 0, 24, B, 19, H, W, pu8.ptr, None, None, s) == -2
    assert l.flair_softmax_argmax_nhwc(x.data_ptr(), 0, 16, B, 17, H, W, pu8.ptr, None, None, s) == -2
    assert l.flair_softmax_argmax_nhwc(x.data_ptr(), 2, 16, B, 13, H, W, pu8.ptr, None, None, s) == -2
    assert l.flair_softmax_argmax_nhwc(None, 0, 16, B, 13, H, W, pu8.ptr, None, None, s) == -1
    torch.cuda.synchronize()
    # nothing ran: every buffer is as it was filled
    for k in ("dl", "preds", "targets", "cm", "loss"):
        g = o[k]
        assert torch.equal(_bits(g.full.cpu()), g.before), k
    assert torch.equal(_bits(ws.full.cpu()), ws.before) and torch.equal(_bits(pu8.full.cpu()), pu8.before)
    assert b"16-byte" in l.flair_strerror(-3)
