"""Every writer of U-Net weights against every cache of the eval forward (case table: eval_cache_cases.py).

``flair_amd.Unet`` keeps two things between eval forwards: the packed weights and BatchNorm coefficients in the eval workspace, reused
while one key stands (reuse_constants of flair_unet_fwd_opts_t), and from the third identical call on a captured HIP graph, which has the addresses
of the flat parameter / buffer tensors baked in.  Each case arms one consumer of those caches, applies one writer, and compares the
next three calls — a full pack, the reuse path, the re-captured graph — bit for bit (the bar the two older cache tests hold) with a
COLD model: a fresh instance loaded from the written model's state_dict that runs once, without graphs.  That every writer changes
the answer at all is asserted on the CPU oracle in test_eval_cache_cases_cpu.py, and here against the armed result.

No test in this file empties the allocator's cache: a stale graph then reads freed but still mapped memory and returns a wrong value,
which is what the comparison is for.
"""
import ctypes as C
import os
import threading

import pytest
import torch

import eval_cache_cases as ec

pytestmark = pytest.mark.gpu

CACHE_STATE = ("key", "graphs", "hits", "nocapture")   # of Unet._eval (an EvalCache)


class _env:
    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        self.old = os.environ.get(self.key)
        os.environ[self.key] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.key, None)
        else:
            os.environ[self.key] = self.old


def _config(classes):
    return {"model_framework": {"model_provider": "SegmentationModelsPytorch",
                                "SegmentationModelsPytorch": {"encoder_decoder": "resnet34_unet", "encoder_weights": None}},
            "use_metadata": True, "channels": list(range(1, ec.IN_CH + 1)), "classes": {i: [1, str(i)] for i in range(classes)}}


@pytest.fixture(scope="module")
def shared(dev):
    """classes -> the model state, the donor state (CPU), the inputs on the device and the metadata encoder: built once per class
    count, never modified."""
    import flair_amd
    built = {}

    def get(classes):
        if classes not in built:
            state = torch.random.get_rng_state()
            torch.manual_seed(7)
            try:
                enc = flair_amd.MetadataMLP()
            finally:
                torch.random.set_rng_state(state)
            inp = {k: v.to(dev) for k, v in ec.inputs(classes).items()}
            big = ec.inputs(classes, ec.FACTORY_SHAPE)
            inp["x512"], inp["mtd512"] = big["x"].to(dev), big["mtd"].to(dev)
            built[classes] = dict(state=ec.model_state(classes, ec.MODEL_SEED), donor=ec.model_state(classes, ec.DONOR_SEED),
                                  inp=inp, enc=enc.to(dev).eval(), classes=classes)
        return built[classes]

    yield get
    built.clear()


def _model(state, dtype, classes, dev):
    import flair_amd
    m = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=ec.IN_CH, classes=classes, compute_dtype=dtype)
    m.load_state_dict(state, strict=True)
    return m.to(dev).eval()


def _consumer(name, m, s):
    """run() -> tuple of tensors (clones) of one call of consumer `name` on the Unet `m`."""
    import flair_amd
    inp = s["inp"]
    x = inp["x"]
    if name in ("logits_reuse", "logits_graph"):
        def run():
            with torch.no_grad():
                return (m(x).clone(),)
    elif name == "preds_prob_graph":
        def run():
            p, q = m.predict_classes(x, want_prob=True)
            return (p.clone(), q.clone())
    elif name == "rows_graph":
        def run():
            return (m.eval_logits(x, bottleneck_rows=inp["rows"]).clone(),)
    elif name == "validate_ce":
        tr = flair_amd.SegTrainer(m, lr=0.0, class_weight=inp["weight"])

        def run():
            tr.val_confmat.zero_()
            loss = tr.validate_step(x, inp["lab"])
            return (loss.view(torch.int32).clone(), tr._val_preds.clone(), tr.val_confmat.clone())
    elif name == "factory_metadata":
        fac = flair_amd.FLAIR_ModelFactory.__new__(flair_amd.FLAIR_ModelFactory)
        torch.nn.Module.__init__(fac)
        fac.model_provider, fac.use_metadata = "SegmentationModelsPytorch", True
        fac.enc, fac.seg_model = s["enc"], m
        fac.eval()

        def run():
            with torch.no_grad():
                return (fac(inp["x512"], inp["mtd512"]).clone(),)
    else:
        raise KeyError(name)
    return run


def _same(a, b):
    return len(a) == len(b) and all(u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(a, b))


def _cold(m, consumer, s, dtype, dev):
    """What a model that has never cached anything computes from the state `m` holds now."""
    fresh = _model(m.state_dict(), dtype, s["classes"], dev)
    with _env("FLAIR_EVAL_GRAPH", "0"):
        out = _consumer(consumer, fresh, s)()
    assert len(fresh._eval.graphs) == 0
    return out


def _arm(m, run, consumer):
    calls, gkey = ec.ARMING[consumer]
    armed = [run() for _ in range(calls)]
    assert all(_same(a, armed[0]) for a in armed[1:])
    assert m._eval.key is not None                       # the reuse path is armed ...
    if gkey is None:
        assert len(m._eval.graphs) == 0
    else:
        assert list(m._eval.graphs) == [gkey]            # ... and so is the graph: nothing passes because nothing was cached
    return armed[0]


def test_factory_shell_is_the_factory(dev, shared):
    """The consumer `factory_metadata` wraps a given Unet in a FLAIR_ModelFactory without building a second network: it must be
    the real class, take the real forward, and compute what a factory built the ordinary way computes."""
    import flair_amd
    s = shared(13)
    real = flair_amd.FLAIR_ModelFactory(_config(13), compute_dtype="f32")
    real.seg_model.load_state_dict(s["state"])
    real.enc.load_state_dict(s["enc"].state_dict())
    real = real.to(dev).eval()
    with torch.no_grad():
        want = real(s["inp"]["x512"], s["inp"]["mtd512"])
    got = _consumer("factory_metadata", _model(s["state"], "f32", 13, dev), s)()
    assert torch.equal(got[0], want)


@pytest.mark.parametrize("writer,consumer,dtype,classes", ec.matrix(), ids=lambda v: str(v))
def test_writer_is_seen_by_consumer(dev, shared, writer, consumer, dtype, classes):
    s = shared(classes)
    hip = _model(s["state"], dtype, classes, dev)
    run = _consumer(consumer, hip, s)
    armed = _arm(hip, run, consumer)
    armed_ptr = (hip._flat_p.data_ptr(), hip._flat_b.data_ptr())
    gkey = ec.ARMING[consumer][1]

    fn = ec.WRITERS[writer]
    made = fn(hip, s["donor"], s["inp"]) if writer in ec.NEEDS_INPUTS else fn(hip, s["donor"])

    if writer in ec.COPY_WRITERS:
        assert made is not hip and made._eval is not hip._eval
        assert [getattr(made._eval, k) for k in CACHE_STATE] == [None, {}, {}, set()]
        made = made.eval()
        subjects = [(made, _consumer(consumer, made, s), True), (hip, run, False)]
    else:
        assert made is None
        subjects = [(hip, run, True)]

    for m, call, written in subjects:
        want = _cold(m, consumer, s, dtype, dev)
        first = call()
        if written:
            # (before the result is read) a written model starts over: no graph of the old state is left, let alone replayed
            assert len(m._eval.graphs) == 0
            if writer in ec.REBUILDING or m is not hip:
                assert m._flat_p.data_ptr() != armed_ptr[0] and m._flat_b.data_ptr() != armed_ptr[1]
        assert _same(first, want), f"{writer} -> {consumer}: first call after the writer"
        assert _same(first, armed) != written, f"{writer}: the answer {'did not change' if written else 'changed'}"
        assert _same(call(), want), f"{writer} -> {consumer}: second call (reuse path)"
        assert _same(call(), want), f"{writer} -> {consumer}: third call (graph, where one is captured)"
        if gkey is not None:
            assert list(m._eval.graphs) == [gkey]


# ------------------------------------------------------------------------------------------------ the C ABI, no Python cache
def test_native_reuse_request_is_refused_for_other_parameter_or_buffer_addresses(dev, shared):
    """reuse_constants is a vouch for the CONTENTS behind the same pointers.  A caller that repeats it with another
    parameter or buffer tensor must get a full pack, not the previous tensor's packed weights / BatchNorm coefficients."""
    from flair_amd import _lib as L
    s = shared(13)
    m = _model(s["state"], "f32", 13, dev)
    l = L.lib()
    x = s["inp"]["x"]
    B, _, H, W = x.shape
    P1, F1 = m.flat_parameters().clone(), m.flat_buffers().clone()
    P2, F2 = P1.clone(), F1.clone()
    (_, off_b, _, _), (shape_w, off_w, _, _) = m._layout["segmentation_head.0.bias"], m._layout["encoder.layer1.0.conv1.weight"]
    P2[off_b + 3] += 1.0
    n_w = 1
    for d in shape_w:
        n_w *= d
    P2[off_w:off_w + n_w] *= 1.5
    _, off_v, kind_v, _ = m._layout["encoder.bn1.running_var"]
    assert kind_v == 1
    F2[off_v:off_v + 64] *= 4.0
    need = l.flair_unet_workspace_bytes(m._h, B, H, W, 0)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    handles = []

    def handle():
        h = C.c_void_p()
        L.check(l.flair_unet_create(C.byref(h), ec.IN_CH, 13, 0), "flair_unet_create")
        handles.append(h)
        return h

    def forward(h, P, F, arena, reuse):
        out = torch.empty(B, 13, H, W, dtype=torch.float32, device=dev)
        opts = L.UnetFwdOpts(reuse_constants=int(reuse))
        L.check(l.flair_unet_forward(h, L.ptr(P), L.ptr(F), L.ptr(x), L.ptr(out), B, H, W, 0, L.ptr(arena), arena.numel(), L.stream(),
                                     C.byref(opts)), "flair_unet_forward")
        return out

    try:
        with torch.cuda.device(dev):
            cold_ws = torch.empty_like(ws)
            cold = {k: forward(handle(), P, F, cold_ws, False) for k, (P, F) in
                    {"11": (P1, F1), "21": (P2, F1), "22": (P2, F2)}.items()}
            assert not torch.equal(cold["11"], cold["21"]) and not torch.equal(cold["21"], cold["22"])
            h = handle()
            assert torch.equal(forward(h, P1, F1, ws, False), cold["11"])
            got = forward(h, P2, F1, ws, True)            # other parameters behind the request
            assert torch.equal(got, cold["21"]), "reuse taken with another params pointer"
            got = forward(h, P2, F2, ws, True)            # other buffers behind the request
            assert torch.equal(got, cold["22"]), "reuse taken with another buffers pointer"
            assert torch.equal(forward(h, P2, F2, ws, True), cold["22"])    # same everything: the reuse path, legitimately
            assert torch.equal(forward(h, P1, F1, ws, True), cold["11"])    # and back
        torch.cuda.synchronize(dev)
    finally:
        for h in handles:
            l.flair_unet_destroy(h)


# ------------------------------------------------------------------------------------------------ capture that fails
def _eager(m, x, calls=1):
    with _env("FLAIR_EVAL_GRAPH", "0"), torch.no_grad():
        outs = [m(x).clone() for _ in range(calls)]
    assert len(m._eval.graphs) == 0
    return outs[-1]


def test_failed_capture_falls_back_to_the_eager_call(dev, shared, monkeypatch):
    """The native call inside the capture raises: that call returns the eager bits, the graph key is marked and later
    calls run eagerly without another attempt."""
    from flair_amd import _lib as L
    s = shared(13)
    m = _model(s["state"], "f32", 13, dev)
    x = s["inp"]["x"]
    want = _eager(m, x)
    m.weights_changed()
    real = L.lib().flair_unet_forward
    attempts = []

    def forward(*args):
        if torch.cuda.is_current_stream_capturing() and not attempts:
            attempts.append(args[-1]._obj.reuse_constants)     # (opts arrives as ctypes.byref(struct))
            raise RuntimeError("planted: the native call of the capture")
        return real(*args)

    monkeypatch.setattr(L.lib(), "flair_unet_forward", forward)
    gkey = (True, False, False, False)
    with torch.no_grad():
        assert torch.equal(m(x), want) and torch.equal(m(x), want)
        with pytest.warns(UserWarning, match="graph capture"):
            third = m(x)
        assert attempts == [1] and torch.equal(third, want)
        assert not torch.cuda.is_current_stream_capturing()
        assert gkey in m._eval.nocapture and len(m._eval.graphs) == 0
        for _ in range(3):
            assert torch.equal(m(x), want)
        assert attempts == [1] and len(m._eval.graphs) == 0
        # another kind of call under the same key is captured as usual
        p = [m.predict_classes(x).clone() for _ in range(3)]
        assert list(m._eval.graphs) == [(False, True, False, False)] and torch.equal(p[0], p[2])
    monkeypatch.undo()
    with torch.no_grad():
        m.weights_changed()                                # a new key: the mark is gone with the old one
        outs = [m(x) for _ in range(3)]
    assert gkey in m._eval.graphs and all(torch.equal(o, want) for o in outs)


def test_capture_survives_another_thread_that_pins_host_memory(dev, shared, monkeypatch):
    """A DataLoader's pin-memory thread allocates page-locked memory whenever it likes.  Here a helper thread does so inside the open
    capture and is joined there: the forward must complete with the eager bits."""
    s = shared(13)
    m = _model(s["state"], "f32", 13, dev)
    x = s["inp"]["x"]
    want = _eager(m, x)
    m.weights_changed()
    pinned = []

    class graph_with_a_pinning_thread(torch.cuda.graph):
        def __enter__(self):
            r = super().__enter__()

            def pin():
                pinned.append(torch.empty(1 << 20, dtype=torch.uint8, pin_memory=True))

            t = threading.Thread(target=pin)
            t.start()
            t.join()
            return r

    monkeypatch.setattr(torch.cuda, "graph", graph_with_a_pinning_thread)
    with torch.no_grad():
        outs = [m(x).clone() for _ in range(4)]
    assert len(pinned) == 1 and pinned[0].is_pinned()
    assert all(torch.equal(o, want) for o in outs)
    assert list(m._eval.graphs) == [(True, False, False, False)]   # thread-local capture mode: the capture itself went through
