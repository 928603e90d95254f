"""Writers of U-Net weights and consumers of the eval forward's caches: the case table of test_gpu_eval_cache.py and of the CPU
preconditions in test_eval_cache_cases_cpu.py.

Between two eval forwards ``flair_amd.Unet`` keeps the packed weights and BatchNorm coefficients in the eval workspace (reuse) and,
from the third identical call on, a captured HIP graph.  A WRITER is one way the weights or running statistics can change between two
such forwards; a CONSUMER is one way those caches are read.  Every writer is a function ``(model, donor_state) -> None`` (the two copy
writers return the copy they made).  Where a writer needs nothing of the HIP model it is written against the module surface the CPU
oracle (oracle.unet_resnet34) shares with it — same module tree, same state_dict keys — and the CPU test applies that very function to
the oracle; a writer that goes through the native library (training forwards, the fused trainer, the flat buffers, pickling of native
state) has an oracle twin in ORACLE_TWINS that makes the same change with torch on the CPU.

Three writers deviate from being the bare call their name says, because a writer that leaves every value as it was can expose no
stale cache: ``cpu_cuda_roundtrip`` swaps the donor tensors in on the host (``.data =``, which moves no version counter, like the
round trip itself), ``double_float_roundtrip`` loads the donor state while the model is fp64, and the copy writers rebind the COPY to
the donor state and leave the original alone.
"""
import copy
import pickle

import torch

IN_CH = 5
SHAPE = (1, IN_CH, 64, 64)            # the smallest extent the suite uses; every cache is armed at it
FACTORY_SHAPE = (1, IN_CH, 512, 512)  # FLAIR_ModelFactory's metadata branch refuses anything else (16 bottleneck rows)
TRAIN_SHAPE = (2, IN_CH, 64, 64)      # the batch of the training-mode writers
MODEL_SEED, DONOR_SEED, INPUT_SEED = 41, 42, 43
SGD_LR = 0.05

FULL = ("f32", 13)                                   # every writer x every consumer
NARROW = (("bf16", 13), ("f32", 19), ("bf16", 19))   # NARROW_WRITERS x NARROW_CONSUMERS only
NARROW_WRITERS = ("rebind_all", "cpu_cuda_roundtrip", "trainer_sgd")
NARROW_CONSUMERS = ("logits_graph", "preds_prob_graph")

CONSUMERS = ("logits_reuse", "logits_graph", "preds_prob_graph", "rows_graph", "validate_ce", "factory_metadata")
# consumer -> (identical calls that arm it, the _eval.graphs entry those calls must have left: (logits, preds, prob, rows) or None)
ARMING = {
    "logits_reuse": (2, None),
    "logits_graph": (4, (True, False, False, False)),
    "preds_prob_graph": (4, (False, True, True, False)),
    "rows_graph": (4, (True, False, False, True)),
    "validate_ce": (2, None),                         # a forward with the CE head is never captured
    "factory_metadata": (4, (True, False, False, True)),
}


def inputs(classes, shape=SHAPE):
    """CPU tensors, the same for every case of one class count: x, a second batch for the training writers and its labels, bottleneck
    rows, uint8 labels and class weights for validate_step, metadata vectors for the factory."""
    g = torch.Generator().manual_seed(INPUT_SEED)
    B, _, H, W = shape
    return dict(
        x=torch.randn(*shape, generator=g),
        x_train=torch.randn(*TRAIN_SHAPE, generator=g),
        lab_train=torch.randint(0, classes, (TRAIN_SHAPE[0],) + TRAIN_SHAPE[2:], generator=g).to(torch.uint8),
        rows=torch.randn(B, H // 32, generator=g),
        lab=torch.randint(0, classes, (B, H, W), generator=g).to(torch.uint8),
        weight=torch.linspace(0.5, 2.0, classes),
        mtd=torch.rand(B, 45, generator=g),
    )


def model_state(classes, seed):
    """state_dict of the seeded CPU oracle with every BatchNorm given a bias, a running mean and a running variance of its own, and
    the head a bias.  As initialised (biases and means 0, variances 1) the network is positively homogeneous: scaling a running
    variance or a weight tensor scales every logit by one factor and moves no argmax, and stale BatchNorm coefficients of two
    states could not be told apart."""
    from oracle import unet_resnet34 as om
    m = om.seeded_model(IN_CH, classes, seed)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.bias.copy_(0.25 * torch.randn(mod.bias.shape, generator=g))
                mod.running_mean.copy_(0.25 * torch.randn(mod.bias.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.bias.shape, generator=g))
        m.segmentation_head[0].bias.copy_(0.25 * torch.randn(classes, generator=g))
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _tensors(m):
    """name -> parameter / buffer, in state_dict order."""
    out = dict(m.named_parameters())
    out.update(dict(m.named_buffers()))
    return out


def _device(m):
    return next(m.parameters()).device


def _on(donor, dev):
    return {k: v.detach().clone().to(dev) for k, v in donor.items()}


def _head_bias(m):
    return m.segmentation_head[0].bias


# ------------------------------------------------------------------------------------------------ writers both models take
@torch.no_grad()
def inplace_param(m, donor):
    m.segmentation_head[0].weight.mul_(-1.5)


@torch.no_grad()
def inplace_buffer(m, donor):
    m.encoder.bn1.running_var.mul_(4)


def load_state_dict(m, donor):
    m.load_state_dict(donor)


def load_state_dict_assign(m, donor):
    m.load_state_dict(_on(donor, _device(m)), assign=True)


def rebind_all(m, donor):
    new = _on(donor, _device(m))   # on the device before the first rebind
    for name, t in _tensors(m).items():
        t.data = new[name]


def rebind_one_param(m, donor):
    """Head bias: + 1 on class 3 and a smaller shift of its own on every other class, so that every logit moves."""
    b = _head_bias(m)
    shift = torch.arange(1, b.numel() + 1, dtype=b.dtype, device=b.device) / (4 * b.numel())
    shift[3] = 1.0
    b.data = b.data + shift


def rebind_one_buffer(m, donor):
    rv = m.encoder.bn1.running_var
    rv.data = 4 * rv.data


def cpu_cuda_roundtrip(m, donor):
    dev = _device(m)
    m.cpu()
    for name, t in _tensors(m).items():
        t.data = donor[name].detach().clone()
    m.to(dev)


def double_float_roundtrip(m, donor):
    m.double()
    m.load_state_dict(donor)
    m.float()


@torch.no_grad()
def data_inplace(m, donor):
    """The write torch's version counters cannot see."""
    m.segmentation_head[0].weight.data.mul_(-1.5)


# ------------------------------------------------------------------------------------------------ writers of the HIP model alone
@torch.no_grad()
def inplace_flat(m, donor):
    m.flat_parameters().mul_(1.125)


def train_forward(m, donor, inp=None):
    was = m.training
    m.train()
    with torch.no_grad():
        m(inp["x_train"])
    m.train(was)


def split_train_encoder(m, donor, inp=None):
    was = m.training
    m.train()
    with torch.no_grad():
        m.encoder(inp["x_train"])
    m.train(was)


def trainer_sgd(m, donor, inp=None):
    import flair_amd
    was = m.training
    tr = flair_amd.SegTrainer(m.train(), lr=SGD_LR)
    tr.train_step(inp["x_train"], inp["lab_train"])
    m.train(was)


def pickle_roundtrip(m, donor):
    blob = pickle.dumps(m)
    state_bytes = sum(t.numel() * t.element_size() for t in _tensors(m).values())
    assert len(blob) < 2 * state_bytes, (len(blob), state_bytes)   # (a view of a flat buffer must not pickle the whole buffer)
    c = pickle.loads(blob)
    rebind_all(c, donor)
    return c


def deepcopy(m, donor):
    c = copy.deepcopy(m)
    rebind_all(c, donor)
    return c


def data_inplace_then_weights_changed(m, donor):
    data_inplace(m, donor)
    m.weights_changed()


WRITERS = {
    "inplace_param": inplace_param,
    "inplace_buffer": inplace_buffer,
    "inplace_flat": inplace_flat,
    "load_state_dict": load_state_dict,
    "load_state_dict_assign": load_state_dict_assign,
    "rebind_all": rebind_all,
    "rebind_one_param": rebind_one_param,
    "rebind_one_buffer": rebind_one_buffer,
    "cpu_cuda_roundtrip": cpu_cuda_roundtrip,
    "double_float_roundtrip": double_float_roundtrip,
    "train_forward": train_forward,
    "split_train_encoder": split_train_encoder,
    "trainer_sgd": trainer_sgd,
    "pickle_roundtrip": pickle_roundtrip,
    "deepcopy": deepcopy,
    "data_inplace_then_weights_changed": data_inplace_then_weights_changed,
}
NEEDS_INPUTS = ("train_forward", "split_train_encoder", "trainer_sgd")
COPY_WRITERS = ("pickle_roundtrip", "deepcopy")
# writers after which flatten_() finds a tensor that no longer aliases the flat buffers and allocates new ones
REBUILDING = ("load_state_dict_assign", "rebind_all", "rebind_one_param", "rebind_one_buffer", "cpu_cuda_roundtrip",
              "double_float_roundtrip")


# ------------------------------------------------------------------------------------------------ oracle twins (torch, CPU)
@torch.no_grad()
def _o_inplace_flat(m, donor, inp):
    for p in m.parameters():
        p.mul_(1.125)


def _o_train_forward(m, donor, inp):
    m.train()
    with torch.no_grad():
        m(inp["x_train"])
    m.eval()


def _o_split_train_encoder(m, donor, inp):
    m.train()
    with torch.no_grad():
        m.encoder(inp["x_train"])
    m.eval()


def _o_trainer_sgd(m, donor, inp):
    from oracle import seg_step
    m.train()
    loss = torch.nn.functional.cross_entropy(m(inp["x_train"]), inp["lab_train"].long())
    loss.backward()
    seg_step.sgd_step_(m.parameters(), SGD_LR)
    m.eval()


def _o_copy(m, donor, inp):
    """What the copy holds after the writer (the original is untouched: its state is the 'before' of the comparison)."""
    rebind_all(m, donor)


ORACLE_TWINS = {
    "inplace_flat": _o_inplace_flat,
    "train_forward": _o_train_forward,
    "split_train_encoder": _o_split_train_encoder,
    "trainer_sgd": _o_trainer_sgd,
    "pickle_roundtrip": _o_copy,
    "deepcopy": _o_copy,
    "data_inplace_then_weights_changed": lambda m, donor, inp: data_inplace(m, donor),
}


def apply_to_oracle(name, m, donor, inp):
    twin = ORACLE_TWINS.get(name)
    if twin is not None:
        return twin(m, donor, inp)
    return WRITERS[name](m, donor)


def matrix():
    """[(writer, consumer, dtype, classes)]: the full product at FULL, the narrow one at each of NARROW."""
    out = [(w, c, *FULL) for w in WRITERS for c in CONSUMERS]
    out += [(w, c, dt, cl) for dt, cl in NARROW for w in NARROW_WRITERS for c in NARROW_CONSUMERS]
    return out
