"""Update rules of the fused trainer: plain and momentum SGD and AdamW over flat buffers.  Every ``SegTrainer`` steps through a
``FlatOptimizer``; without ``optimizer=`` its specification is ``SGD()``, the reference's rule, which has no state buffers.

``SGD`` and ``AdamW`` are specifications: hyper-parameters without tensors, validated by torch.optim's own rules and messages.
``FlatOptimizer`` binds one to a flat fp32 parameter buffer, to state buffers of the same length allocated beside it and to the
ordered ``nn.Parameter`` views of that buffer; its ``step`` is one HIP kernel over the whole buffer (csrc/optim.hip: no per-tensor
launches, no host sync).  ``TrainerOptimizer`` is what ``SegTrainer.optimizer`` exposes when a rule was asked for: ``state_dict()`` /
``load_state_dict()`` in torch.optim's format over a chosen parameter order, so ``checkpoint.save_checkpoint`` / ``resume`` and
``torch.optim.SGD`` / ``AdamW`` exchange state with the fused trainer.

The learning rate is not part of a specification: the trainer's ``lr`` is the live one (a scheduler sets it), and a step takes it
as an argument.  Out of scope: per-group hyper-parameters, amsgrad, maximize, low-precision state.
"""
from __future__ import annotations

import torch


class SGD:
    """torch.optim.SGD's rule: g' = g + wd p;  buf = g' (first step) | mu buf + (1 - dampening) g';  g' = g' + mu buf (nesterov) |
    buf;  p -= lr g'."""
    name = "sgd"
    state_keys = ("momentum_buffer",)

    def __init__(self, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.momentum, self.dampening, self.weight_decay, self.nesterov = float(momentum), float(dampening), float(weight_decay), bool(nesterov)

    @property
    def n_state(self):
        return 1 if self.momentum != 0 else 0

    def torch_optimizer(self, params, lr):
        return torch.optim.SGD(params, lr=lr, momentum=self.momentum, dampening=self.dampening, weight_decay=self.weight_decay,
                               nesterov=self.nesterov)

    def __repr__(self):
        return f"SGD(momentum={self.momentum}, dampening={self.dampening}, weight_decay={self.weight_decay}, nesterov={self.nesterov})"


class AdamW:
    """torch.optim.AdamW's rule (decoupled decay, no amsgrad, no maximize): p *= 1 - lr wd;  m += (g - m)(1 - b1);
    v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)."""
    name = "adamw"
    state_keys = ("exp_avg", "exp_avg_sq")
    n_state = 2

    def __init__(self, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        betas = tuple(betas)
        if len(betas) != 2:
            raise ValueError(f"betas must be a pair, got {betas!r}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)

    def torch_optimizer(self, params, lr):
        return torch.optim.AdamW(params, lr=lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)

    def __repr__(self):
        return f"AdamW(betas={self.betas}, eps={self.eps}, weight_decay={self.weight_decay})"


_BY_NAME = {"sgd": SGD, "adamw": AdamW}


def from_config(config):
    """The specification of the config's optional ``optimizer: {name: sgd|adamw, ...}`` key (the other entries are the class's
    arguments); without the key the reference's rule, plain SGD (tasks_utils.py:95)."""
    entry = config.get("optimizer")
    if entry is None:
        return SGD()
    if not isinstance(entry, dict) or "name" not in entry:
        raise ValueError("config['optimizer'] must be a mapping with a 'name' (sgd or adamw)")
    kw = {k: v for k, v in entry.items() if k != "name"}
    name = str(entry["name"]).lower()
    if name not in _BY_NAME:
        raise ValueError(f"unknown optimizer {entry['name']!r} (use 'sgd' or 'adamw')")
    if "lr" in kw:
        raise ValueError("the learning rate is config['learning_rate'], not an entry of config['optimizer']")
    return _BY_NAME[name](**kw)


def torch_optimizer_from_config(config, params):
    """The torch.optim object of the same key for the LightningModule surface; without the key exactly
    ``torch.optim.SGD(params, lr=config['learning_rate'])``."""
    if config.get("optimizer") is None:
        return torch.optim.SGD(params, lr=config["learning_rate"])
    return from_config(config).torch_optimizer(params, config["learning_rate"])


def _step_number(v):
    return int(v.item()) if isinstance(v, torch.Tensor) else int(v)


class FlatOptimizer:
    """One specification over one flat fp32 parameter buffer.  ``params``: the ordered ``nn.Parameter``s whose data are views of
    ``flat`` (offset of p = (p.data_ptr() - flat.data_ptr()) / 4).  The state buffers are zero-initialised, as long as ``flat``
    and indexed like it, so the state of a parameter is the same slice of them."""

    def __init__(self, spec, flat, params):
        if flat.dtype != torch.float32 or flat.dim() != 1 or not flat.is_contiguous():
            raise ValueError("FlatOptimizer takes a contiguous 1-d fp32 parameter buffer")
        self.spec = spec
        self.flat = flat
        self.params = list(params)
        self.state = [torch.zeros_like(flat) for _ in range(spec.n_state)]
        self.steps = 0   # steps taken (torch's per-parameter ``step``: every bound parameter steps together)
        for p in self.params:
            self.offset(p)

    def offset(self, p):
        d = p.data_ptr() - self.flat.data_ptr()
        if p.dtype != torch.float32 or not p.is_contiguous() or d % 4 or d < 0 or d // 4 + p.numel() > self.flat.numel():
            raise ValueError("parameter is not a contiguous fp32 view of the flat buffer")
        return d // 4

    def step(self, grads, lr, grad_scale=1.0, coef=None):
        """One update of the whole buffer from the flat gradient: g' = grads * grad_scale * coef (``coef``: a device float)."""
        from . import ops
        s = self.spec
        first = self.steps == 0
        if s.name == "sgd":
            ops.optim_sgd_(self.flat, grads, self.state[0] if self.state else None, lr, momentum=s.momentum, dampening=s.dampening,
                           weight_decay=s.weight_decay, nesterov=s.nesterov, first=first, grad_scale=grad_scale, coef=coef)
        else:
            ops.optim_adamw_(self.flat, grads, self.state[0], self.state[1], lr, betas=s.betas, eps=s.eps, weight_decay=s.weight_decay,
                             step=self.steps + 1, first=first, grad_scale=grad_scale, coef=coef)
        self.steps += 1

    # ---- torch.optim's per-parameter state
    def param_state(self, p):
        """{} before the first step (and for plain SGD, which has none), else clones shaped like ``p``."""
        if self.steps == 0 or (self.spec.name == "sgd" and not self.state):
            return {}
        o, n = self.offset(p), p.numel()
        out = {}
        if self.spec.name == "adamw":
            out["step"] = torch.tensor(float(self.steps), dtype=torch.float32)
        for key, buf in zip(self.spec.state_keys, self.state):
            out[key] = buf[o:o + n].view(p.shape).clone()
        return out

    def load_param_states(self, states):
        """``states``: one torch.optim state mapping ({} = none yet) per bound parameter, in ``params`` order."""
        if len(states) != len(self.params):
            raise ValueError("one state per bound parameter")
        steps = set()
        for p, st in zip(self.params, states):
            have = bool(st) and all(st.get(k) is not None for k in self.spec.state_keys)
            if not have:
                steps.add(0)
                continue
            steps.add(_step_number(st["step"]) if "step" in st else -1)
        if len(steps - {-1}) > 1 or (0 in steps and len(steps) > 1):
            raise ValueError("a flat optimizer steps all its parameters together: the states' step counts differ")
        if not self.state:
            self.steps = 0
            return
        if steps == {0}:
            self.steps = 0
            for buf in self.state:
                buf.zero_()
            return
        with torch.no_grad():
            for p, st in zip(self.params, states):
                o, n = self.offset(p), p.numel()
                for key, buf in zip(self.spec.state_keys, self.state):
                    t = st[key]
                    if tuple(t.shape) != tuple(p.shape):
                        raise ValueError(f"state {key} has shape {tuple(t.shape)}, its parameter {tuple(p.shape)}")
                    buf[o:o + n].view(p.shape).copy_(t)
        known = steps - {-1}
        self.steps = known.pop() if known else max(self.steps, 1)   # momentum SGD keeps no count: any step but the first


class TrainerOptimizer:
    """``SegTrainer.optimizer``: the trainer's flat optimizers seen as one torch.optim-style object over ``params`` (an ordered
    parameter list; parameters no flat optimizer holds simply have no state, like parameters torch never saw a gradient of)."""

    def __init__(self, spec, flat_optimizers, params, lr_of, set_lr=None):
        self.spec = spec
        self.flat_optimizers = flat_optimizers   # a callable: the bound FlatOptimizers of the moment
        self.params = list(params)
        self._lr_of, self._set_lr = lr_of, set_lr

    def _owner(self):
        own = {}
        for fo in self.flat_optimizers():
            for p in fo.params:
                own[id(p)] = fo
        return own

    def _group(self):
        # key names and defaults of the installed torch, from torch itself
        ref = self.spec.torch_optimizer([torch.nn.Parameter(torch.zeros(1))], self._lr_of())
        group = dict(ref.state_dict()["param_groups"][0])
        group["params"] = list(range(len(self.params)))
        return group

    def state_dict(self):
        own = self._owner()
        state = {}
        for i, p in enumerate(self.params):
            fo = own.get(id(p))
            st = fo.param_state(p) if fo is not None else {}
            if st:
                state[i] = st
        return {"state": state, "param_groups": [self._group()]}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1:
            raise ValueError("the fused trainer keeps one parameter group")
        ids = list(groups[0]["params"])
        if len(ids) != len(self.params):
            raise ValueError(f"loaded state dict has {len(ids)} parameters, the trainer's parameter list {len(self.params)}")
        mine = self._group()
        for k, v in groups[0].items():
            if k in ("params", "lr") or k not in mine:
                continue
            a, b = (tuple(v), tuple(mine[k])) if isinstance(v, (list, tuple)) else (v, mine[k])
            if a != b and k in ("momentum", "dampening", "weight_decay", "nesterov", "betas", "eps", "amsgrad", "maximize"):
                raise ValueError(f"loaded state dict was written with {k}={v!r}, the trainer's optimizer has {mine[k]!r}")
        by_param = {id(p): sd["state"].get(i, {}) for p, i in zip(self.params, ids)}
        for fo in self.flat_optimizers():
            fo.load_param_states([by_param.get(id(p), {}) for p in fo.params])
        if self._set_lr is not None and "lr" in groups[0]:
            self._set_lr(float(groups[0]["lr"]))   # torch restores the group's learning rate with the state
