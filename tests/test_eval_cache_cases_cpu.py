"""CPU preconditions of test_gpu_eval_cache.py (no device needed).

(a) The torch semantics the eval key of ``flair_amd.Unet`` leans on, and the collision the key had while it held version counters
    only: ``flatten_()``'s copy-and-rebind (``flair_amd.flat``) runs on a Conv2d and a BatchNorm2d.
(b) Every writer of eval_cache_cases really changes the answer — judged on the CPU oracle alone, so that a GPU case cannot pass
    because the stale and the fresh result happen to coincide.
"""
import copy

import pytest
import torch
import torch.nn as nn

import eval_cache_cases as ec
from flair_amd import flat


# ------------------------------------------------------------------------------------------------ (a) what the key can see
class _Flat:
    """``Unet.flatten_`` without the native library, over the binder it uses: parameters -> one flat buffer, running statistics ->
    another, every tensor rebound as a ``.data`` view; both rebuilt when a tensor no longer aliases its slot."""

    def __init__(self):
        self.mods = nn.ModuleList([nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4)])
        # running statistics that no in-place op has written yet (BatchNorm2d's own reset fills them in place): Module._apply
        # REPLACES a buffer by a new tensor, whose counter starts at 0, where it rebinds a parameter's .data and keeps its counter
        self.mods[1].running_mean = torch.zeros(4)
        self.mods[1].running_var = torch.ones(4)
        self.flat_p = self.flat_b = None
        self.layout = []
        offs = [0, 0]
        for name, t in list(self.mods.named_parameters()) + [(n, b) for n, b in self.mods.named_buffers() if b.dtype == torch.float32]:
            kind = 0 if isinstance(t, nn.Parameter) else 1
            self.layout.append((name, kind, offs[kind], tuple(t.shape)))
            offs[kind] += t.numel()
        self.n = offs

    def tensor(self, name):
        mod = self.mods
        *path, leaf = name.split(".")
        for p in path:
            mod = mod[int(p)]
        return getattr(mod, leaf)

    def flatten_(self):
        items = [[(self.tensor(name), off, shape) for name, kind, off, shape in self.layout if kind == k] for k in (0, 1)]
        if all(flat.aliased(f, (i[:2] for i in its)) for f, its in zip((self.flat_p, self.flat_b), items)):
            return False
        self.flat_p, self.flat_b = (flat.bind(its, n, "cpu") for its, n in zip(items, self.n))
        return True

    def versions(self):
        ts = list(self.mods.parameters()) + list(self.mods.buffers())
        return (sum(t._version for t in ts), self.flat_p._version, self.flat_b._version)

    def addresses(self):
        return (self.flat_p.data_ptr(), self.flat_b.data_ptr())


def test_data_assignment_moves_no_version_counter():
    p = nn.Parameter(torch.zeros(4))
    with torch.no_grad():
        p.mul_(2)
    v = p._version
    assert v == 1
    p.data = torch.ones(4)
    assert p._version == v and float(p.detach().sum()) == 4.0
    p.data.mul_(3)                       # in place through .data: the one write nothing can see
    assert p._version == v and float(p.detach().sum()) == 12.0
    with torch.no_grad():
        p.mul_(1)
    assert p._version == v + 1


def _rebind_all(f):
    for name, _, _, _ in f.layout:
        t = f.tensor(name)
        t.data = t.data * 2 + 1


def _apply_roundtrip(f):
    f.mods.double()
    f.mods.float()


@pytest.mark.parametrize("writer", [_rebind_all, _apply_roundtrip], ids=["rebind_all", "apply_roundtrip"])
def test_a_key_of_versions_alone_collides_where_one_with_addresses_does_not(writer):
    f = _Flat()
    assert f.flatten_() and not f.flatten_()
    old = (f.flat_p, f.flat_b)           # (kept alive: the addresses cannot be handed out again)
    versions, addresses = f.versions(), f.addresses()
    before = f.flat_p.clone()
    writer(f)
    assert f.flatten_()                  # the writer unhooked the tensors: new flat buffers
    assert f.flat_p is not old[0] and f.flat_b is not old[1]
    # a rebuilt flat buffer repeats the version of the one it replaces: one copy_ per tensor
    assert f.flat_p._version == versions[1] == sum(1 for _, k, _, _ in f.layout if k == 0)
    assert f.flat_b._version == versions[2] == sum(1 for _, k, _, _ in f.layout if k == 1)
    assert f.versions() == versions                                   # the old key: equal, although ...
    assert f.addresses()[0] != addresses[0] and f.addresses()[1] != addresses[1]   # ... every address moved
    assert (f.versions() + f.addresses()) != (versions + addresses)   # the key with addresses tells them apart
    if writer is _rebind_all:
        assert not torch.equal(f.flat_p, before)                      # and so did the values


def test_bind_copies_every_tensor_to_its_offset_and_aliased_tells_when_one_left():
    mods = nn.ModuleList([nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4)])
    ts = list(mods.parameters())
    offs, o = [], 5                                   # a gap in front, and one of 3 floats behind every tensor
    for t in ts:
        offs.append(o)
        o += t.numel() + 3
    want = [t.detach().clone() for t in ts]
    items = lambda: list(zip(ts, offs))
    buf = flat.bind([(t, off, t.shape) for t, off in items()], o, "cpu")
    assert buf.dtype == torch.float32 and tuple(buf.shape) == (o,) and buf._version == len(ts)   # one copy_ per tensor
    used = torch.zeros(o, dtype=torch.bool)
    for t, off, w in zip(ts, offs, want):
        assert torch.equal(t.detach(), w) and t.data_ptr() == buf.data_ptr() + 4 * off
        assert torch.equal(buf[off:off + t.numel()].view(t.shape), w)
        used[off:off + t.numel()] = True
    assert int((~used).sum()) == 5 + 3 * len(ts) and not bool(buf[~used].any())    # the gaps stay zero
    assert flat.aliased(buf, items())
    with torch.no_grad():
        for t in ts:
            t.mul_(2)                                 # in-place writes go through the views
    assert flat.aliased(buf, items()) and torch.equal(buf[offs[0]:offs[0] + ts[0].numel()].view(ts[0].shape), 2 * want[0])
    assert not flat.aliased(None, items())
    assert not flat.aliased(buf, [(t, off + (i == 1)) for i, (t, off) in enumerate(items())])     # an offset off by one
    keep = ts[2].data
    ts[2].data = keep.clone()                         # one tensor rebound
    assert not flat.aliased(buf, items())
    ts[2].data = keep
    assert flat.aliased(buf, items())
    mods.double()                                     # (parameters keep their identity: Module._apply rebinds .data)
    assert not flat.aliased(buf, items())


# ------------------------------------------------------------------------------------------------ (b) every writer matters
@pytest.fixture(scope="module")
def oracle_case():
    from oracle import unet_resnet34 as om
    classes = ec.FULL[1]
    model = om.create_model("unet", "resnet34", in_channels=ec.IN_CH, classes=classes).eval()
    model.load_state_dict(ec.model_state(classes, ec.MODEL_SEED))
    donor = ec.model_state(classes, ec.DONOR_SEED)
    inp = ec.inputs(classes)
    with torch.no_grad():
        before = model(inp["x"])
    return dict(state=copy.deepcopy(model.state_dict()), donor=donor, inp=inp, before=before, classes=classes)


@pytest.mark.parametrize("writer", list(ec.WRITERS))
def test_writer_changes_the_answer_on_the_oracle(oracle_case, writer):
    from oracle import unet_resnet34 as om
    c = oracle_case
    m = om.create_model("unet", "resnet34", in_channels=ec.IN_CH, classes=c["classes"])
    m.load_state_dict(c["state"])
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(c["inp"]["x"]), c["before"])              # same state, same answer: the comparison starts level
    ec.apply_to_oracle(writer, m, c["donor"], c["inp"])
    assert not m.training
    with torch.no_grad():
        after = m(c["inp"]["x"]).float()
    assert after.dtype == torch.float32 and torch.isfinite(after).all()
    changed = float((after != c["before"]).float().mean())
    flips = int((after.argmax(1) != c["before"].argmax(1)).sum())
    print(f"{writer}: {100 * changed:.2f} % of the logits differ, {flips} of {after[:, 0].numel()} mask pixels")
    assert changed >= 0.99
    assert flips >= 1


def test_the_case_table_is_what_the_gpu_test_expects():
    assert set(ec.ARMING) == set(ec.CONSUMERS)
    assert set(ec.ORACLE_TWINS) | set(ec.REBUILDING) <= set(ec.WRITERS)
    assert set(ec.NARROW_WRITERS) <= set(ec.WRITERS) and set(ec.NARROW_CONSUMERS) <= set(ec.CONSUMERS)
    assert len(ec.matrix()) == len(ec.WRITERS) * len(ec.CONSUMERS) + len(ec.NARROW) * len(ec.NARROW_WRITERS) * len(ec.NARROW_CONSUMERS)
