"""Host state of the U-Net mirror, without a device: the decisions of the eval cache (flair_amd.unet.EvalCache) driven with
made-up keys, the declared native state of ``Unet`` through construction and pickling, and NativeModel's version bookkeeping."""
import copy
import pickle

import pytest
import torch

GK = (True, False, False, False)        # a logits call
GK2 = (False, True, True, False)        # a preds + probability call


def _cache():
    from flair_amd.unet import EvalCache
    return EvalCache()


def _call(c, key, gkey=GK, has_ce=False, pixels=64 * 64, graphs_allowed=True, capturing=False, captures=True):
    """One eval forward as Unet._c_forward drives the cache: the decision it acted on, as 'full' / 'reuse' / 'capture' / 'replay',
    or 'failed' for a capture that broke (the call then runs as a full pack)."""
    todo = c.decide(key, gkey, has_ce, pixels, graphs_allowed, capturing)
    if todo == c.GRAPH:
        if gkey in c.graphs:
            return "replay"
        if captures:
            c.graphs[gkey] = object()
            return "capture"
        c.capture_failed(gkey)
        c.packed(key)
        return "failed"
    c.packed(key)
    return {c.FULL: "full", c.REUSE: "reuse"}[todo]


def test_full_then_reuse_then_capture_then_replay():
    c = _cache()
    assert (c.key, c.graphs, c.hits, c.nocapture) == (None, {}, {}, set())
    assert [_call(c, ("k", 1)) for _ in range(5)] == ["full", "reuse", "capture", "replay", "replay"]
    assert list(c.graphs) == [GK] and c.hits == {GK: 4} and c.key is not None
    # another kind of call under the same key counts for itself: the constants are there, its graph is not
    assert [_call(c, ("k", 1), GK2) for _ in range(3)] == ["reuse", "capture", "replay"]
    assert list(c.graphs) == [GK, GK2]
    assert _call(c, ("k", 1)) == "replay"


def test_key_change_starts_over():
    c = _cache()
    for _ in range(4):
        _call(c, ("k", 1))
    assert _call(c, ("k", 2)) == "full"
    assert (c.graphs, c.hits, c.nocapture) == ({}, {}, set())
    assert [_call(c, ("k", 2)) for _ in range(3)] == ["reuse", "capture", "replay"]
    assert _call(c, ("k", 1)) == "full"                       # back to an earlier key: nothing of it was kept


def test_native_write_changes_the_key_and_drop_empties():
    c = _cache()
    for _ in range(4):
        _call(c, ("k", 1))
    c.note_native_write()                                      # same caller key, but a native writer has run
    assert [_call(c, ("k", 1)) for _ in range(4)] == ["full", "reuse", "capture", "replay"]
    c.drop()                                                   # weights_changed() / rebuilt flat buffers
    assert (c.key, c.graphs, c.hits, c.nocapture) == (None, {}, {}, set())
    assert [_call(c, ("k", 1)) for _ in range(3)] == ["full", "reuse", "capture"]
    c.key = None                                               # the split path: constants gone, everything goes with the next call
    assert _call(c, ("k", 1)) == "full" and c.graphs == {}


def test_failed_capture_marks_its_kind_until_the_key_changes():
    c = _cache()
    assert [_call(c, ("k", 1), captures=False) for _ in range(3)] == ["full", "reuse", "failed"]
    assert c.nocapture == {GK} and c.graphs == {}
    # marked: eager with reuse from now on, no further attempt (the 'failed' call itself packed again)
    assert [_call(c, ("k", 1)) for _ in range(3)] == ["reuse"] * 3
    assert [_call(c, ("k", 1), GK2) for _ in range(3)] == ["reuse", "capture", "replay"]     # other kinds are captured as usual
    assert _call(c, ("k", 2)) == "full" and c.nocapture == set()
    assert [_call(c, ("k", 2)) for _ in range(2)] == ["reuse", "capture"]


def test_ce_calls_are_not_counted_and_never_captured():
    c = _cache()
    assert [_call(c, ("k", 1), has_ce=True) for _ in range(5)] == ["full"] + ["reuse"] * 4
    assert c.hits == {} and c.graphs == {}
    # the plain call of the same graph key still needs its own two repeats
    assert [_call(c, ("k", 1)) for _ in range(2)] == ["reuse", "capture"]
    assert _call(c, ("k", 1), has_ce=True) == "reuse"          # ... and a CE call does not replay that graph


@pytest.mark.parametrize("off", [dict(graphs_allowed=False), dict(capturing=True), dict(pixels=4 * 512 * 512 + 1)],
                         ids=["FLAIR_EVAL_GRAPH=0", "capture-open", "pixel-limit"])
def test_no_graph_when_switched_off_too_large_or_inside_a_capture(off):
    c = _cache()
    assert [_call(c, ("k", 1), **off) for _ in range(5)] == ["full"] + ["reuse"] * 4
    assert c.hits == {} and c.graphs == {}
    assert [_call(c, ("k", 1)) for _ in range(3)] == ["reuse", "capture", "replay"]
    assert _call(c, ("k", 1), **off) == "reuse"                # an existing graph is not replayed either


def test_pixel_limit_is_inclusive():
    c = _cache()
    assert c.MAX_GRAPH_PIXELS == 4 * 512 * 512
    assert [_call(c, ("k", 1), pixels=c.MAX_GRAPH_PIXELS) for _ in range(3)] == ["full", "reuse", "capture"]


# ------------------------------------------------------------------------------------------------ declared state
def _plain_attrs(m):
    return {k for k in m.__dict__ if k not in ("_modules", "_parameters", "_buffers")}


def test_native_state_is_declared_in_one_place():
    import flair_amd
    from flair_amd.unet import EvalCache
    m = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=13)
    declared = set(m._native_state)
    assert {"_h", "_h_eval", "_flat_p", "_flat_b", "_flat_n", "_ws", "_ws_need", "_eval", "_live"} <= declared
    assert m._h_eval is None and m._flat_n is None and isinstance(m._eval, EvalCache)

    # what the reset method assigns is what it says it assigns ...
    bare = flair_amd.Unet.__new__(flair_amd.Unet)
    torch.nn.Module.__init__(bare)
    bare.in_channels, bare.classes, bare._dt = m.in_channels, m.classes, m._dt
    before = set(bare.__dict__)
    bare._reset_native_state()
    assert set(bare.__dict__) - before == declared | {"_native_state"}
    # ... pickling drops exactly that ...
    assert _plain_attrs(m) - set(m.__getstate__()) == declared
    # ... and the copies have the same attributes as a fresh model, every declared one newly made
    for c in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert _plain_attrs(c) == _plain_attrs(m)
        assert c._native_state == m._native_state
        assert c._h.value != m._h.value and c._eval is not m._eval and c._live is not m._live and c._ws is not m._ws
        assert (c._eval.key, c._eval.graphs, c._eval.hits, c._eval.nocapture) == (None, {}, {}, set())
        assert c.encoder._owner is c and c._layout == m._layout
        assert all(torch.equal(a, b) for a, b in zip(c.state_dict().values(), m.state_dict().values()))


def test_earlier_attribute_names_forward_to_the_new_objects():
    """_eval_graphs, _eval_nocapture, _eval_key and _live_ws are properties of the class: no state of their own, nothing in __dict__."""
    import flair_amd
    m = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=13)
    assert m._eval_graphs is m._eval.graphs and m._eval_nocapture is m._eval.nocapture and m._live_ws is m._live.ws
    m._eval.packed(("k", 1))
    assert m._eval_key is m._eval.key is not None
    m._eval_key = None
    assert m._eval.key is None
    assert not {"_eval_graphs", "_eval_nocapture", "_eval_key", "_live_ws"} & set(m.__dict__)


def test_native_models_do_not_shadow_module_version():
    """nn.Module._version is the class's state_dict format version (load_state_dict reads it from the metadata)."""
    import flair_amd
    from flair_amd._native_model import NativeModel
    from flair_amd.upernet import config_for_upernet
    models = (flair_amd.SegformerForSemanticSegmentation(num_channels=5, num_labels=19),
              flair_amd.UperNetForSemanticSegmentation(num_channels=3, num_labels=19, **config_for_upernet("openmmlab/upernet-swin-tiny")))
    for m in models:
        assert isinstance(m, NativeModel)
        assert "_version" not in m.__dict__ and m._version == torch.nn.Module._version
        assert m._seen_version == -1                           # (its own counter: nothing flattened yet)
        assert m.state_dict()._metadata[""]["version"] == torch.nn.Module._version
