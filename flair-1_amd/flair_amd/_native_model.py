"""Host-side base of the native inference models (segformer.py, upernet.py): an ``nn.Module`` tree of PARAMETER CONTAINERS over one
flat fp32 device buffer laid out by the native tensor table.  All arithmetic runs in libflair_hip.so; host tensors are refused.

The library keeps packed copies of the weights between forwards, so this class also owns the protocol that tells it when they are
stale (``_flatten``: tensor version counters).  A subclass sets ``_PREFIX`` (its C symbols are ``flair_<_PREFIX>_*``), creates the
native handle, and allocates the outputs of its own forward.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib as L
from . import flat as _flat


def tensor_of(root, name):
    """(module, leaf) of the dotted parameter / buffer name under ``root`` (digits index Sequential / ModuleList children)."""
    mod = root
    *path, leaf = name.split(".")
    for p in path:
        mod = mod._modules[p]
    return mod, leaf


def query_layout(num_tensors, tensor_info, h, stage=False):
    """The native tensor table of handle ``h``: name -> (shape, float offset, kind) and, with ``stage``, the gradient stage."""
    out = {}
    name = C.create_string_buffer(160)
    shape = (C.c_int64 * 4)()
    nd, kind, st, off = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    extra = (C.byref(st),) if stage else ()
    for i in range(num_tensors(h)):
        L.check(tensor_info(h, i, name, 160, shape, C.byref(nd), C.byref(off), C.byref(kind), *extra))
        out[name.value.decode()] = (tuple(shape[d] for d in range(nd.value)), off.value, kind.value) + ((st.value,) if stage else ())
    return out


class _Box(nn.Module):
    """A node of the parameter tree (children are added by dotted name)."""

    def forward(self, *a, **k):
        raise RuntimeError("flair_amd: sub-modules are parameter containers; call the model")


class NativeModel(nn.Module):
    _PREFIX = ""                # "segformer" / "upernet"
    _ZERO_LEAVES = ("bias",)    # parameters that start at zero
    _BAD_TILE = ""              # the unsupported-tile-size message, formatted with H and W

    def _fn(self, name):
        return getattr(L.lib(), f"flair_{self._PREFIX}_{name}")

    def _init_tensors(self, h, initializer_range):
        """Takes the native handle: builds the parameter tree from its tensor table, initialised like the library."""
        object.__setattr__(self, "_h", h)
        self._layout = query_layout(self._fn("num_tensors"), self._fn("tensor_info"), h)
        self._n = self._fn("param_count")(h)
        g = torch.Generator().manual_seed(torch.initial_seed() & 0x7FFFFFFF)
        for name, (shape, off, kind) in self._layout.items():
            leaf = name.rsplit(".", 1)[1]
            if kind == 1:
                t = torch.zeros(shape) if leaf == "running_mean" else torch.ones(shape)
            elif leaf in self._ZERO_LEAVES:
                t = torch.zeros(shape)
            elif len(shape) == 1:            # LayerNorm / BatchNorm weight
                t = torch.ones(shape)
            else:                             # Linear / Conv2d weight: normal(0, initializer_range) like the library
                t = torch.empty(shape).normal_(0.0, initializer_range, generator=g)
            self._attach(name, t, kind)
            if leaf == "running_var":        # BatchNorm2d's counter follows its running statistics in the library's order
                self._attach(name[:-len("running_var")] + "num_batches_tracked", torch.zeros((), dtype=torch.int64), 1)
        self._flat = None
        self._seen_version = -1
        self._ws = None

    # ---- parameter tree
    def _attach(self, name, tensor, kind):
        mod = self
        *path, leaf = name.split(".")
        for p in path:
            if p not in mod._modules:
                mod.add_module(p, _Box())
            mod = mod._modules[p]
        if kind == 0:
            mod.register_parameter(leaf, nn.Parameter(tensor, requires_grad=False))
        else:
            mod.register_buffer(leaf, tensor)

    def train(self, mode=True):
        if mode:
            raise RuntimeError(f"flair_amd.{type(self).__name__} is inference-only (zone_detect never trains)")
        return super().train(False)

    def _flatten(self):
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise L.FlairHipError(f"flair_amd.{type(self).__name__} runs on a HIP device only: call .cuda() first")
        items = [(getattr(*tensor_of(self, name)), off, shape) for name, (shape, off, _) in self._layout.items()]
        if _flat.aliased(self._flat, (i[:2] for i in items)):
            version = sum(t._version for t, _, _ in items)
            if version != self._seen_version:   # an in-place update (load_state_dict, copy_, ...) since the last forward:
                self.weights_changed()          # the library re-packs its cached weight layouts
                self._seen_version = version
            return self._flat
        self._flat = _flat.bind(items, self._n, dev)
        self._seen_version = sum(t._version for t, _, _ in items)
        self.weights_changed()
        return self._flat

    def weights_changed(self):
        """The library keeps packed copies of the weights between forwards; in-place updates through the module's parameters are
        noticed (tensor version counters), updates through ``.data`` or raw pointers are not — call this after such an update."""
        self._fn("weights_changed")(self._h)

    # ---- native forward
    def _prepare(self, x):
        """Checks the input, flattens the parameters and sizes the workspace: (flat parameters, fp32 contiguous input).  The caller
        allocates its outputs and calls the native forward under ``torch.cuda.device(flat.device)``."""
        if not x.is_cuda:
            raise L.FlairHipError(f"flair_amd.{type(self).__name__} needs HIP tensors (no CPU fallback)")
        flat = self._flatten()
        if x.device != flat.device:
            raise L.FlairHipError(f"tensor on {x.device} passed to a model on {flat.device}")
        x = x.detach().to(torch.float32).contiguous()
        if x.dim() != 4 or x.shape[1] != self.num_channels:
            raise RuntimeError(f"expected input (B,{self.num_channels},H,W), got {tuple(x.shape)}")
        B, _, H, W = x.shape
        with torch.cuda.device(flat.device):
            need = self._fn("workspace_bytes")(self._h, B, H, W)
            if need <= 0:
                raise RuntimeError(self._BAD_TILE.format(H=H, W=W))
            if self._ws is None or self._ws.numel() < need or self._ws.device != flat.device:
                self._ws = torch.empty(need, dtype=torch.uint8, device=flat.device)
        return flat, x

    def __del__(self):
        try:
            h = self.__dict__.get("_h")
            if h:
                self._fn("destroy")(h)
        except Exception:  # noqa: BLE001
            pass
