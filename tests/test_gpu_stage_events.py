"""The seven stage events of flair_unet_backward: an event may fire only when its stage's slice of the flat gradient buffer is
FINAL.  The data-parallel exchange (SegTrainer.train_step) starts a bucket's all-reduce on another stream the moment the event
fires, while the rest of the backward is still running; a weight-gradient reduction, a BatchNorm-backward finalize or a bias
column sum that lands behind its stage's event would be read half-written by RCCL, and no single-GPU test would notice (a gloo
all-reduce goes through the host and starts long after anything late has landed).

Here a stream of the test's own stands in for the exchange: it waits for each event in ready order (head 6, decoder 5, layer4
... layer1, stem 0) and copies the stage's slice at once.  The buffer holds NaN before every backward, so a late write shows as a
NaN (or, on an element written twice, as a different value) in the snapshot.  This is the most adversarial timing available
without RCCL: the copy is queued behind nothing but the event.  A pass does NOT prove that no race exists — a write that is
late by less than the copy's own launch latency goes unseen — it proves that the ordering the code states is the ordering the
streams keep: every stage's kernels lie in front of the position its event was recorded at.

Paths of UNet::stage_done (csrc/unet.hip) that run here:
  * third stream: stages 1-6 by default and under FLAIR_NOTE_PRIO=0 / 2 (the note stream at the caller's / the highest priority);
  * plain record on the caller's stream: stage 0 always (behind side_join), every stage under FLAIR_WGRAD_STREAM=0.
The side_join fallback inside stage_done runs only when the third stream cannot be created; no switch reaches it, so it has no
test."""
import contextlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TUNE_DEFAULTS = {"FLAIR_WGRAD_STREAM": 1, "FLAIR_NOTE_PRIO": 1}
SETTINGS = {"default": {}, "wgrad_stream_off": {"FLAIR_WGRAD_STREAM": 0}, "note_prio_0": {"FLAIR_NOTE_PRIO": 0},
            "note_prio_2": {"FLAIR_NOTE_PRIO": 2}}
READY_ORDER = (6, 5, 4, 3, 2, 1, 0)
PASSES = 3   # ~60 recycled fork events per pass (47 weight-gradient forks + 2 per stage 1-6): the ring of 128 wraps in the third


@contextlib.contextmanager
def _tune(pairs):
    from flair_amd import _lib as L
    try:
        for k, v in pairs.items():
            L.check(L.lib().flair_tune_set(k.encode(), v))
        yield
    finally:
        for k, v in TUNE_DEFAULTS.items():
            L.lib().flair_tune_set(k.encode(), v)


def _model(dev, dtype, seed=9):
    """A fresh HIP model with the oracle's seeded weights (the side and note streams are created once per native handle)."""
    import flair_amd
    from oracle import unet_resnet34 as om
    hip = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=13, compute_dtype=dtype)
    hip.load_state_dict(om.seeded_model(5, 13, seed).state_dict(), strict=True)
    return hip.to(dev).train()


def _batch(dev):
    """Batch Y of test_step_does_not_see_the_previous_steps_partial_sums (4 x 5 x 128 x 192, drawn behind X and before the labels)."""
    g = torch.Generator().manual_seed(3)
    torch.randn(4, 5, 128, 192, generator=g)
    y = torch.randn(4, 5, 128, 192, generator=g)
    torch.randint(0, 13, (4, 128, 192), generator=g)
    ly = torch.randint(0, 13, (4, 128, 192), generator=g).to(torch.uint8)
    return y.to(dev), ly.to(dev)


def _bits(t):
    return t.view(torch.int32)   # NaN-proof, sign-of-zero-proof equality


def _parameter_mask(m, n):
    """True where the flat buffer holds a parameter.  The rest is alignment padding (every stage begins at a multiple of four
    floats, csrc/unet.hip build_table): no kernel owns those elements, they are legitimately never written."""
    mask = torch.zeros(n, dtype=torch.bool)
    for name in m._param_names:
        shape, off, kind, _ = m._layout[name]
        assert kind == 0 and not mask[off:off + math.prod(shape)].any()   # parameters do not overlap
        mask[off:off + math.prod(shape)] = True
    return mask


def _step(m, x, dl, G, events):
    m._c_forward(x, training=True, want_logits=False)
    m._c_backward(dlogits_nhwc=dl, grads=G, stage_events=events)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stage_event_fires_only_when_its_gradient_slice_is_final(dev, dtype, setting):
    import flair_amd
    with _tune(SETTINGS[setting]):
        m = _model(dev, dtype)
        x, lab = _batch(dev)
        tr = flair_amd.SegTrainer(m, lr=0.0)      # the trainer's own d(loss)/d(logits), NHWC rows of the compute dtype
        tr.train_step(x, lab)
        dl = tr._dl
        ranges = m.stage_ranges()
        n = tr.grads.numel()
        assert ranges[0][0] == 0 and ranges[6][1] == n and all(ranges[s][1] == ranges[s + 1][0] for s in range(6))
        mask = _parameter_mask(m, n).to(dev)
        # the padding: at most three floats behind a stage, and for 13 classes only behind the head (16*13*9 + 13 = 1885 -> 1888)
        pad = (~mask).nonzero().flatten().tolist()
        assert pad == [n - 3, n - 2, n - 1], pad

        # reference: the same step into a zero-filled buffer, events recorded
        events = [torch.cuda.Event() for _ in range(7)]
        for e in events:
            e.record()   # materialise the handles, as SegTrainer.__init__ does
        G0 = torch.zeros(n, dtype=torch.float32, device=dev)
        _step(m, x, dl, G0, events)
        torch.cuda.synchronize()
        assert not torch.isnan(G0).any() and float(G0.abs().max()) > 0
        assert torch.equal(_bits(G0), _bits(tr.grads))          # the direct calls repeat the trainer's step

        snap_stream = torch.cuda.Stream(device=dev)
        G = torch.empty(n, dtype=torch.float32, device=dev)
        # nothing but the event may stand between a stage's last kernel and its copy: the snapshots' memory exists before the
        # first pass (an allocation behind the wait synchronises the device) and the snapshot stream has already run kernels
        # (a stream's first launch sets up its hardware queue, milliseconds in which the whole backward finishes)
        snap = {stage: torch.empty(e - b, dtype=torch.float32, device=dev) for stage, (b, e) in enumerate(ranges)}
        for p in range(PASSES):                                  # the SAME seven events every pass
            with torch.cuda.stream(snap_stream):
                for t in snap.values():
                    t.zero_()
            torch.cuda.synchronize()
            G.fill_(float("nan"))
            _step(m, x, dl, G, events)
            with torch.cuda.stream(snap_stream):
                for stage in READY_ORDER:
                    snap_stream.wait_event(events[stage])        # must wait for THIS pass's record, not be satisfied by the last one's
                    b, e = ranges[stage]
                    snap[stage].copy_(G[b:e])
            torch.cuda.synchronize()
            for stage in READY_ORDER:
                b, e = ranges[stage]
                diff = _bits(snap[stage]) != _bits(G[b:e])
                assert not diff.any(), (p, stage, int(diff.sum()), int(torch.isnan(snap[stage]).sum()),
                                        (b + diff.nonzero().flatten()[:8]).tolist())
            # every parameter's gradient written, nothing accumulated into what the buffer held, padding untouched
            assert not torch.isnan(G[mask]).any(), (p, int(torch.isnan(G[mask]).sum()))
            assert torch.isnan(G[~mask]).all() and not G0[~mask].any()
            assert torch.equal(_bits(G[mask]), _bits(G0[mask])), p

        # the events do not change the arithmetic (same setting, same grids)
        G.fill_(float("nan"))
        _step(m, x, dl, G, None)
        torch.cuda.synchronize()
        assert torch.equal(_bits(G[mask]), _bits(G0[mask])) and torch.isnan(G[~mask]).all()
