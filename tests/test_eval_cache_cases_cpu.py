"""CPU preconditions of test_gpu_eval_cache.py (no device needed).

(a) The torch semantics the eval key of ``flair_amd.Unet`` leans on, and the collision the key had while it held version counters
    only: ``flatten_()``'s copy-and-rebind is replayed on a Conv2d and a BatchNorm2d.
(b) Every writer of eval_cache_cases really changes the answer — judged on the CPU oracle alone, so that a GPU case cannot pass
    because the stale and the fresh result happen to coincide.
"""
import copy

import pytest
import torch
import torch.nn as nn

import eval_cache_cases as ec


# ------------------------------------------------------------------------------------------------ (a) what the key can see
class _Flat:
    """``Unet.flatten_`` without the native library: parameters -> one flat buffer, running statistics -> another, every tensor
    rebound as a ``.data`` view; rebuilt when a tensor no longer aliases its slot."""

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
        ok = self.flat_p is not None
        if ok:
            for name, kind, off, _ in self.layout:
                t = self.tensor(name)
                if t.data_ptr() != (self.flat_p, self.flat_b)[kind].data_ptr() + 4 * off or t.dtype != torch.float32:
                    ok = False
                    break
        if ok:
            return False
        flat = [torch.zeros(self.n[0]), torch.zeros(self.n[1])]
        with torch.no_grad():
            for name, kind, off, shape in self.layout:
                t = self.tensor(name)
                view = flat[kind][off:off + t.numel()].view(shape)
                view.copy_(t.detach().to(torch.float32))
                t.data = view
        self.flat_p, self.flat_b = flat
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
