"""Host-side mirror of ``segmentation_models_pytorch.Unet('resnet34')`` over the HIP executor.

Drop-in for the object ``smp.create_model(arch='unet', encoder_name='resnet34', classes, in_channels)``
returns at /root/reference/src/flair/model.py:37-41 (contract: SURVEY.md §8b):

* ``forward(x) -> logits`` (B,classes,H,W) fp32, H and W divisible by 32 else RuntimeError;
* ``.encoder(x) -> list`` of 6 features, ``.decoder(*feats)``, ``.segmentation_head(t)`` (model.py:57-62);
* ``.parameters()`` are leaf ``nn.Parameter``s (fp32, PyTorch OIHW) that receive ``.grad``;
* ``state_dict()`` / ``load_state_dict()`` use the smp-0.3.3 key names and shapes;
* ``.modules()`` contains real ``nn.BatchNorm2d`` objects (src/flair/tasks.py:25-26 looks for them);
* ``train()`` / ``eval()`` switch BatchNorm between batch and running statistics.

The nn.Conv2d / nn.BatchNorm2d sub-modules are PARAMETER CONTAINERS only: all arithmetic runs in
libflair_hip.so on the current HIP stream.  Host tensors are refused (there is no CPU fallback).
Parameters and BN running statistics live in two flat fp32 device buffers (views per tensor) whose
layout the native library defines (``flair_unet_tensor_info``); stage-contiguous gradients make the
bucketed RCCL all-reduce of ``flair_amd.train`` possible.
"""
from __future__ import annotations

import copy
import ctypes as C
import functools
import math
import os
import warnings

import torch
import torch.nn as nn

from . import _lib as L
from . import flat as _flat
from ._native_model import query_layout, tensor_of
from .tta import tta_codes, tta_predict


def _on_model_device(fn):
    """Native calls launch on the CURRENT device's stream and the library's internal streams / events are created on the
    current device: run them with the model's device current (a model on cuda:1 while cuda:0 is current — two replicas in
    one process, a forgotten set_device — would otherwise launch on the wrong device's stream), and refuse inputs that
    live elsewhere."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        dev = self._flat_p.device if self._flat_p is not None else None
        if dev is None or dev.type != "cuda":
            return fn(self, *args, **kwargs)
        for a in args:
            ts = a if isinstance(a, (list, tuple)) else (a,)
            for t in ts:
                if torch.is_tensor(t) and t.is_cuda and t.device != dev:
                    raise L.FlairHipError(f"tensor on {t.device} passed to a model on {dev}")
        with torch.cuda.device(dev):
            return fn(self, *args, **kwargs)
    return wrapper


# ------------------------------------------------------------------------------------------------ containers
def _container_forward(self, *a, **k):
    raise RuntimeError("flair_amd: sub-modules are parameter containers; call the Unet / encoder / decoder / head")


class _BasicBlock(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
        self.stride = stride

    forward = _container_forward


class _Encoder(nn.Module):
    """smp ``ResNetEncoder('resnet34')`` key layout; ``__call__`` runs the HIP encoder stage."""

    def __init__(self, owner, in_channels):
        super().__init__()
        object.__setattr__(self, "_owner", owner)
        self.conv1 = nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inpl = 64
        for li, (planes, n) in enumerate(zip((64, 128, 256, 512), (3, 4, 6, 3)), start=1):
            blocks = []
            for b in range(n):
                stride = 2 if (b == 0 and li > 1) else 1
                blocks.append(_BasicBlock(inpl, planes, stride, downsample=(b == 0 and li > 1)))
                inpl = planes
            setattr(self, f"layer{li}", nn.Sequential(*blocks))
        self._out_channels = (in_channels, 64, 64, 128, 256, 512)
        self._depth = 5
        self._in_channels = in_channels

    @property
    def out_channels(self):
        return self._out_channels

    def forward(self, x):
        return self._owner._encoder_forward(x)


class _DecoderBlock(nn.Module):
    def __init__(self, cin, cskip, cout):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(cin + cskip, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))
        self.attention1 = nn.Identity()
        self.conv2 = nn.Sequential(nn.Conv2d(cout, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))
        self.attention2 = nn.Identity()

    forward = _container_forward


class _Decoder(nn.Module):
    def __init__(self, owner):
        super().__init__()
        object.__setattr__(self, "_owner", owner)
        self.center = nn.Identity()
        cin, cskip, cout = (512, 256, 128, 64, 32), (256, 128, 64, 64, 0), (256, 128, 64, 32, 16)
        self.blocks = nn.ModuleList(_DecoderBlock(a, b, c) for a, b, c in zip(cin, cskip, cout))

    def forward(self, *features):
        return self._owner._decoder_forward(*features)


class _Head(nn.Sequential):
    def __init__(self, owner, classes):
        super().__init__(nn.Conv2d(16, classes, 3, padding=1), nn.Identity(), nn.Identity())
        object.__setattr__(self, "_owner", owner)

    def forward(self, x):
        return self._owner._head_forward(x)


# ------------------------------------------------------------------------------------------------ autograd glue
class _WholeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, x, *params):
        logits = owner._c_forward(x, training=True)
        ctx.owner = owner
        ctx.fwd_id = owner._live.id
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        owner = ctx.owner
        owner._check_live(ctx.fwd_id)
        grads = owner._c_backward(dlogits.contiguous())
        return (None, None) + tuple(owner._grad_views(grads))


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, x, *params):
        feats = owner._c_encoder_forward(x, training=True)
        ctx.owner = owner
        ctx.fwd_id = owner._live.id
        return tuple(feats)

    @staticmethod
    def backward(ctx, *dfeats):
        owner = ctx.owner
        owner._check_live(ctx.fwd_id)
        owner._c_encoder_backward([d.contiguous() for d in dfeats])
        return (None, None) + tuple(owner._grad_views(owner._live.grads, "encoder"))


class _DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, f1, f2, f3, f4, f5, *params):
        out = owner._c_decoder_forward([f1, f2, f3, f4, f5], training=True)
        ctx.owner = owner
        ctx.fwd_id = owner._live.id
        return out

    @staticmethod
    def backward(ctx, dout):
        owner = ctx.owner
        owner._check_live(ctx.fwd_id)
        dfeats = owner._c_decoder_backward(dout.contiguous())
        return (None,) + tuple(dfeats) + tuple(owner._grad_views(owner._live.grads, "decoder"))


class _HeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, x, *params):
        logits = owner._c_head_forward(x, training=True)
        ctx.owner = owner
        ctx.fwd_id = owner._live.id
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        owner = ctx.owner
        owner._check_live(ctx.fwd_id)
        dx = owner._c_head_backward(dlogits.contiguous())
        return (None, dx) + tuple(owner._grad_views(owner._live.grads, "segmentation_head"))


# ------------------------------------------------------------------------------------------------ host state
class _LiveForward:
    """The training forward that awaits its backward: its number (``_check_live``), the workspace its activations are in, (B, H, W),
    the (rows, drows) pair the native side holds raw pointers to until that backward, and the split path's gradient buffer."""
    __slots__ = ("id", "ws", "shape", "rows", "grads")

    def __init__(self, id=0, ws=None, shape=None, rows=None):   # (no forward has number 0)
        self.id, self.ws, self.shape, self.rows, self.grads = id, ws, shape, rows, None


class EvalCache:
    """What eval forwards keep between calls, and the decision what the next one does (plain Python, no device call).  ``key`` vouches
    for the packed weights and BatchNorm coefficients in the eval workspace; ``graphs`` holds one captured HIP graph per kind of call
    (graph key: (want_logits, preds, prob, rows)), ``hits`` the repeats of each kind under the key, ``nocapture`` the kinds whose capture
    failed: all four go when the key changes.  The caller's key is extended by the count of native writes (``note_native_write``):
    changes no torch version counter sees — training forwards (running statistics) and the fused trainer's SGD (parameters)."""
    FULL, REUSE, GRAPH = "full", "reuse", "graph"
    # eval forwards of small batches are launch-bound (~150 kernels of a few microseconds: predict_step at the reference's
    # batch size 1, data_module.py:100, ran at 870 tiles/s against 10 000 at batch 32): the third identical call — same weights,
    # shape, workspace and requested outputs — is captured into a HIP graph and replayed from then on (FLAIR_EVAL_GRAPH=0: never)
    MAX_GRAPH_PIXELS = 4 * 512 * 512

    def __init__(self):
        self._native_writes = 0
        self.drop()

    def drop(self):
        """No key (the next eval forward packs again) and no graph captured under it."""
        self.key, self.graphs, self.hits, self.nocapture = None, {}, {}, set()

    def note_native_write(self):
        self._native_writes += 1

    def decide(self, key, gkey, has_ce, pixels, graphs_allowed, capturing):
        """FULL: pack the constants and run eagerly.  REUSE: run eagerly over the constants in the workspace.  GRAPH: replay the
        graph of ``gkey``, capturing it first if there is none — the third identical call, the first repeat having run eagerly with
        reuse so that every kernel's one-time set-up is done.  A call with the CE head neither counts nor is captured."""
        if self.key != (key, self._native_writes):
            self.drop()
            return self.FULL
        if has_ce or not graphs_allowed or pixels > self.MAX_GRAPH_PIXELS or capturing:
            return self.REUSE
        self.hits[gkey] = self.hits.get(gkey, 0) + 1
        return self.GRAPH if gkey not in self.nocapture and (gkey in self.graphs or self.hits[gkey] >= 2) else self.REUSE

    def capture_failed(self, gkey):
        """This kind of call stays eager until the key changes (and runs now as FULL: the broken capture advanced the executor's state)."""
        self.nocapture.add(gkey)

    def packed(self, key):
        """An eager eval forward under ``key`` is being issued: from here on the constants in the workspace are that key's."""
        self.key = (key, self._native_writes)


# ------------------------------------------------------------------------------------------------ the model
class Unet(nn.Module):
    """MI355X-native ``smp.Unet(encoder_name='resnet34')``.

    Extra keyword (not in smp): ``compute_dtype`` = 'f32' (parity mode: exact-fp32 MFMA, the
    reference trains in fp32, src/flair/tasks.py:83-93) or 'bf16' (throughput mode).  Default comes
    from the environment variable FLAIR_AMD_DTYPE, else 'f32'.
    """

    def __init__(self, encoder_name="resnet34", encoder_depth=5, encoder_weights="imagenet", decoder_use_batchnorm=True,
                 decoder_channels=(256, 128, 64, 32, 16), decoder_attention_type=None, in_channels=3, classes=1,
                 activation=None, aux_params=None, compute_dtype=None):
        super().__init__()
        if encoder_name != "resnet34":
            raise KeyError(f"Wrong encoder name `{encoder_name}`, supported encoders: ['resnet34']")
        if (encoder_depth != 5 or not decoder_use_batchnorm or tuple(decoder_channels) != (256, 128, 64, 32, 16)
                or decoder_attention_type is not None or activation is not None or aux_params is not None):
            raise ValueError("flair_amd.Unet implements the configuration the reference uses: smp defaults with resnet34")
        self._dt = L.dtype_code(compute_dtype if compute_dtype is not None else os.environ.get("FLAIR_AMD_DTYPE", "f32"))
        self.in_channels, self.classes = int(in_channels), int(classes)
        self.encoder = _Encoder(self, self.in_channels)
        self.decoder = _Decoder(self)
        self.segmentation_head = _Head(self, self.classes)
        self.classification_head = None
        self.name = "u-resnet34"
        self._init_weights(encoder_weights)
        # native handle + layout
        self._reset_native_state()
        self._layout = query_layout(L.lib().flair_unet_num_tensors, L.lib().flair_unet_tensor_info, self._h, stage=True)
        sd_tensors = {**dict(self.named_parameters()), **dict(self.named_buffers())}
        for name, (shape, off, kind, stage) in self._layout.items():
            t = sd_tensors.get(name)
            if t is None or tuple(t.shape) != shape:
                raise RuntimeError(f"layout mismatch for {name}: native {shape} vs module {None if t is None else tuple(t.shape)}")
        self._param_names = [n for n, (_, _, k, _) in self._layout.items() if k == 0]
        self._buffer_names = [n for n, (_, _, k, _) in self._layout.items() if k == 1]
        self._n_params = L.lib().flair_unet_param_count(self._h)
        self._n_buffers = L.lib().flair_unet_buffer_count(self._h)
        # BatchNorm layers in modules() order, the order of _flat_n: the encoder's, then the decoder's
        self._n_bn_encoder = sum(n.startswith("encoder.") and n.endswith(".running_mean") for n in self._buffer_names)

    def _new_handle(self):
        h = C.c_void_p()
        L.check(L.lib().flair_unet_create(C.byref(h), self.in_channels, self.classes, self._dt), "flair_unet_create")
        return h

    # the names these had before EvalCache / _LiveForward, for code that still reads them
    _eval_graphs = property(lambda self: self._eval.graphs)
    _eval_nocapture = property(lambda self: self._eval.nocapture)
    _eval_key = property(lambda self: self._eval.key, lambda self, key: setattr(self._eval, "key", key))
    _live_ws = property(lambda self: self._live.ws)

    def _reset_native_state(self):
        """Every attribute that holds native or device state, as a model has it before its first forward.  __init__ and
        __setstate__ call this and nothing else creates such an attribute; __getstate__ drops exactly these."""
        state = dict(_h=self._new_handle(), _h_eval=None,         # native executors: training, and eval (made at its first use: _hh)
                     _flat_p=None, _flat_b=None, _flat_n=None,    # flat device buffers: parameters, running statistics, num_batches_tracked
                     _ws={}, _ws_need={},                         # workspaces by mode, and their planned sizes by (B, H, W, training)
                     _eval=EvalCache(), _live=_LiveForward(),
                     _eval_split=None)   # ((B, H, W), workspace) of the eval-mode split forward: it must not disturb _live
        self.__dict__.update(state)
        self._native_state = tuple(state)

    # -------------------------------------------------------------------------------------------- init
    def _init_weights(self, encoder_weights):
        """smp-0.3.3 initialisation: torchvision ResNet init (encoder), kaiming-uniform decoder, xavier head."""
        first = self.encoder.conv1
        for m in self.encoder.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if self.in_channels != 3:
            first.reset_parameters()  # smp patch_first_conv(pretrained=False)
        for m in self.decoder.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, mode="fan_in", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        nn.init.xavier_uniform_(self.segmentation_head[0].weight)
        nn.init.constant_(self.segmentation_head[0].bias, 0)
        if encoder_weights is not None:
            path = os.environ.get("FLAIR_RESNET34_WEIGHTS")
            if path and os.path.isfile(path):
                self.load_encoder_weights(torch.load(path, map_location="cpu", weights_only=True))
            else:
                warnings.warn(
                    f"encoder_weights={encoder_weights!r}: pretrained ResNet34 weights cannot be downloaded here; "
                    "set FLAIR_RESNET34_WEIGHTS=<torchvision resnet34 state_dict .pth> or pass encoder_weights=None. "
                    "Using the seeded random initialisation.")

    def load_encoder_weights(self, sd):
        """torchvision resnet34 state_dict -> encoder, with smp ``patch_first_conv`` for in_channels != 3."""
        sd = {k: v for k, v in sd.items() if not k.startswith("fc.")}
        w = sd["conv1.weight"]
        if self.in_channels == 1:
            sd["conv1.weight"] = w.sum(1, keepdim=True)
        elif self.in_channels != 3:
            nw = torch.empty(w.shape[0], self.in_channels, *w.shape[2:])
            for i in range(self.in_channels):
                nw[:, i] = w[:, i % 3]
            sd["conv1.weight"] = nw * (3 / self.in_channels)
        self.encoder.load_state_dict(sd, strict=True)

    # -------------------------------------------------------------------------------------------- layout
    def stage_ranges(self):
        """[(begin, end)] float offsets of the 7 gradient buckets (stem, layer1-4, decoder, head)."""
        b, e = C.c_int64(), C.c_int64()
        res = []
        for s in range(7):
            L.check(L.lib().flair_unet_stage_range(self._h, s, C.byref(b), C.byref(e)))
            res.append((b.value, e.value))
        return res

    def flatten_(self):
        """(Re)bind every parameter / running statistic as a view of the two flat device buffers."""
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise L.FlairHipError("flair_amd.Unet runs on a HIP device only: call .cuda() first (no CPU fallback)")
        # (tensor, float offset, shape) of the parameters and of the running statistics
        params, buffers = ([(getattr(*tensor_of(self, name)), self._layout[name][1], self._layout[name][0]) for name in names]
                           for names in (self._param_names, self._buffer_names))
        if _flat.aliased(self._flat_p, (i[:2] for i in params)) and _flat.aliased(self._flat_b, (i[:2] for i in buffers)):
            return
        flat_p = _flat.bind(params, self._n_params, dev)
        flat_b = _flat.bind(buffers, max(self._n_buffers, 1), dev)
        with torch.no_grad():
            bns = [m for m in self.modules() if isinstance(m, nn.BatchNorm2d)]
            flat_n = torch.zeros(len(bns), dtype=torch.int64, device=dev)
            for i, m in enumerate(bns):
                flat_n[i] = m.num_batches_tracked.to(dev)
                m.num_batches_tracked.data = flat_n[i]
        self._flat_p, self._flat_b, self._flat_n = flat_p, flat_b, flat_n
        # new buffers repeat the version counters of the ones they replace (one copy_ per tensor) and `.data =` moves none:
        # what was packed from, or captured with, the old addresses goes here, not by a key that may compare equal
        self._eval.drop()

    def weights_changed(self):
        """Announce a change of parameters or running statistics that torch's version counters cannot see — an in-place write
        through ``.data`` (``p.data.mul_(...)``) or through a raw pointer: the next eval forward packs the weights again and
        captures no graph before its third identical call.  Every other writer (in-place torch ops, ``load_state_dict``,
        ``.data =`` / ``.to()`` / ``.cpu()`` rebinds, training forwards, the fused trainer) is noticed without it."""
        self._eval.drop()

    def _eval_cache_key(self, B, H, W, ws):
        """What must be unchanged for the constants in the eval workspace, and a graph captured over them, to be still valid.
        Versions: torch bumps a tensor's _version on every in-place write (optimizers, load_state_dict); the parameters and
        buffers are .data views of the flat buffers and each carries its own counter.  Addresses of the flat buffers: a rebuilt
        buffer repeats its predecessor's versions, and a captured graph has the addresses baked in.  (Native writers: EvalCache.)"""
        ver = sum(p._version for p in self.parameters()) + sum(b._version for b in self.buffers())
        return (ver, self._flat_p._version, self._flat_b._version, self._flat_p.data_ptr(), self._flat_b.data_ptr(), B, H, W, ws.data_ptr())

    def flat_parameters(self):
        self.flatten_()
        return self._flat_p

    def flat_buffers(self):
        self.flatten_()
        return self._flat_b

    def _params_list(self, prefix=None):
        names = [n for n in self._param_names if prefix is None or n.startswith(prefix + ".")]
        return names, [getattr(*tensor_of(self, n)) for n in names]

    def _grad_views(self, grads, prefix=None):
        views = []
        for n in self._param_names:
            if prefix is not None and not n.startswith(prefix + "."):
                continue
            shape, off, _, _ = self._layout[n]
            views.append(grads[off:off + math.prod(shape)].view(shape))
        return views

    # -------------------------------------------------------------------------------------------- native calls
    def _hh(self, training):
        """The native executor for this call: eval-mode forwards (predict, validation, ZoneDetector) run on a second
        handle, so that one issued between a training forward and its backward — legal in PyTorch — leaves the recorded
        training graph alone."""
        if training:
            return self._h
        if self._h_eval is None:
            self._h_eval = self._new_handle()
        return self._h_eval

    def _workspace(self, B, H, W, training):
        key = "train" if training else "eval"
        plan = self._ws_need
        need = plan.get((B, H, W, bool(training)))
        if need is None:   # the dry run walks the whole 47-conv graph on the host: once per shape, not once per step
            need = L.lib().flair_unet_workspace_bytes(self._h, B, H, W, int(training))
            if need < 0:
                raise RuntimeError("flair_unet_workspace_bytes failed")
            plan[(B, H, W, bool(training))] = need
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need or ws.device != self._flat_p.device:
            self._ws[key] = ws = torch.empty(need, dtype=torch.uint8, device=self._flat_p.device)
        return ws

    def check_input_shape(self, x):
        h, w = x.shape[-2:]
        if h % 32 != 0 or w % 32 != 0:
            nh = (h // 32 + 1) * 32 if h % 32 else h
            nw = (w // 32 + 1) * 32 if w % 32 else w
            raise RuntimeError(f"Wrong input shape height={h}, width={w}. Expected image height and width "
                               f"divisible by 32. Consider pad your images to shape ({nh}, {nw}).")

    def _prep(self, x):
        if not x.is_cuda:
            raise L.FlairHipError("flair_amd.Unet needs HIP tensors (no CPU fallback)")
        self.flatten_()
        x = x.detach().to(torch.float32).contiguous()
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise RuntimeError(f"expected input (B,{self.in_channels},H,W), got {tuple(x.shape)}")
        self.check_input_shape(x)
        return x

    def _bump_bn(self, lo=0, hi=None):
        """num_batches_tracked += 1 for BatchNorm layers [lo, hi) (one op on the flat int64 buffer)."""
        self._flat_n[lo:hi] += 1

    _NOT_CAPTURED = object()

    def _eval_graph(self, gkey, x, want_logits, preds, prob, ws, h, rows=None):
        ent = self._eval.graphs.get(gkey)
        if ent is None:
            B, _, H, W = x.shape
            ent = {"x": x.clone(), "logits": torch.empty(B, self.classes, H, W, dtype=torch.float32, device=x.device) if want_logits else None,
                   "preds": None if preds is None else torch.empty_like(preds), "prob": None if prob is None else torch.empty_like(prob),
                   "rows": None if rows is None else rows.clone()}
            g = torch.cuda.CUDAGraph()
            l = L.lib()
            try:
                # thread_local: another thread of the process (a DataLoader's pin-memory thread allocating page-locked memory)
                # may call the runtime while this one captures; under the default mode that call fails and the capture with it
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    opts = self._fwd_opts(True, ent["preds"], ent["prob"], None, ent["rows"], None)
                    L.check(l.flair_unet_forward(h, L.ptr(self._flat_p), L.ptr(self._flat_b), L.ptr(ent["x"]), L.ptr(ent["logits"]), B, H, W, 0,
                                                 L.ptr(ws), ws.numel(), L.stream(), C.byref(opts)), "flair_unet_forward")
            except Exception as e:
                # nothing ran (capture records); the caller runs this same call eagerly, and this kind of call stays eager until
                # the key changes
                warnings.warn(f"flair_amd.Unet: HIP graph capture of the eval forward failed ({type(e).__name__}: {e}); running eagerly")
                self._eval.capture_failed(gkey)
                return self._NOT_CAPTURED
            ent["graph"] = g
            self._eval.graphs[gkey] = ent
        ent["x"].copy_(x)       # (capture records, it does not run: the first use replays too)
        if rows is not None:
            ent["rows"].copy_(rows)
        ent["graph"].replay()
        if preds is not None:
            preds.copy_(ent["preds"])
            if prob is not None:
                prob.copy_(ent["prob"])
        return None if ent["logits"] is None else ent["logits"].clone()

    @staticmethod
    def _fwd_opts(reuse, preds, prob, ce, rows, train_rows):
        """The flair_unet_fwd_opts_t of one native forward.  It holds raw device pointers: the caller keeps the tensors alive."""
        o = L.UnetFwdOpts(reuse_constants=int(reuse))
        if preds is not None:
            o.preds_u8, o.maxprob_f32 = L.ptr(preds), L.ptr(prob)
        if ce is not None:
            o.ce_labels, o.ce_label_kind, o.ce_class_weight, o.ce_loss, o.ce_preds_u8, o.ce_confmat, o.ce_workspace = ce
        if train_rows is not None:
            rows, o.drows_f32 = train_rows[0], L.ptr(train_rows[1])
        o.rows_f32 = L.ptr(rows)
        return o

    @_on_model_device
    def _c_forward(self, x, training, want_logits=True, preds=None, prob=None, ce=None, rows=None, train_rows=None):
        """want_logits=False (fused trainer): the head's output stays in the workspace as NHWC rows of the compute dtype
        (flair_unet_logits_nhwc) and no fp32 NCHW tensor is produced; returns None.  preds / prob (eval mode, no logits): uint8
        argmax and its fp32 probability from the head convolution's epilogue (flair_unet_fwd_opts_t::preds_u8).  ce (eval mode, no
        logits): the seven ce_ fields of flair_unet_fwd_opts_t in their order — the validation head in the same call; such a forward
        always runs eagerly (never captured, not counted towards the captures of the plain paths).  rows (eval mode only): fp32
        (B, H/32) added to the bottleneck feature between encoder and decoder, element [b,c,h,w] += rows[b,h]
        (rows_f32 of the options) — the metadata fusion of model.py:57-62 inside the one native call; combines with all of the above.
        train_rows (training mode only, excludes rows): a pair (rows, drows) of fp32 (B, H/32) tensors — the same add in a training
        forward, out of place (rows_f32 + drows_f32); the _c_backward of this forward writes d loss / d rows into drows."""
        x = self._prep(x)
        B, _, H, W = x.shape
        if train_rows is not None:
            if rows is not None:
                raise RuntimeError("flair_amd.Unet: rows= (eval mode) and train_rows= (training mode) exclude each other")
            if not training:
                raise RuntimeError("flair_amd.Unet: train_rows= is for training-mode forwards; an eval-mode forward takes rows=")
            t_rows, t_drows = train_rows
            self._check_rows(t_rows, x)
            self._check_rows(t_drows, x)
            if t_drows.dtype != torch.float32 or not t_drows.is_contiguous():
                raise RuntimeError("flair_amd.Unet: the gradient tensor of train_rows must be contiguous fp32 (the backward writes it)")
            train_rows = (t_rows.detach().to(torch.float32).contiguous(), t_drows.detach())
        if rows is not None:
            if training:
                raise RuntimeError("flair_amd.Unet: bottleneck rows are added in eval-mode forwards only; a training-mode model "
                                   "takes the split path (encoder, add, decoder, segmentation_head)")
            self._check_rows(rows, x)
            rows = rows.detach().to(torch.float32).contiguous()
        ws = self._workspace(B, H, W, training)
        h = self._hh(training)
        # constant weights between two eval forwards (predict / zone_detect loops): skip the weight pack and the
        # BatchNorm-coefficient launches while the key (_eval_cache_key) stands.  Writes through .data are invisible to it,
        # as they are to autograd: weights_changed() is the call for those.
        reuse = False
        if not training:
            key = self._eval_cache_key(B, H, W, ws)
            gkey = (want_logits, preds is not None, prob is not None, rows is not None)
            todo = self._eval.decide(key, gkey, ce is not None, B * H * W, os.environ.get("FLAIR_EVAL_GRAPH", "1") != "0",
                                torch.cuda.is_current_stream_capturing())
            if todo == self._eval.GRAPH:
                out = self._eval_graph(gkey, x, want_logits, preds, prob, ws, h, rows)
                if out is not self._NOT_CAPTURED:
                    return out
                todo = self._eval.FULL   # (EvalCache.capture_failed: this call packs again)
            reuse = todo == self._eval.REUSE
        logits = torch.empty(B, self.classes, H, W, dtype=torch.float32, device=x.device) if want_logits else None
        opts = self._fwd_opts(reuse, preds, prob, ce, rows, train_rows)
        if not training:
            self._eval.packed(key)
        else:
            self._eval.note_native_write()   # running statistics are about to change
        L.check(L.lib().flair_unet_forward(h, L.ptr(self._flat_p), L.ptr(self._flat_b), L.ptr(x), L.ptr(logits), B, H, W,
                                           int(training), L.ptr(ws), ws.numel(), L.stream(), C.byref(opts)), "flair_unet_forward")
        if training:
            # (rows: the native side holds raw pointers until the backward of this forward)
            self._live = _LiveForward(self._live.id + 1, ws, (B, H, W), train_rows)
            self._bump_bn()
        return logits

    @staticmethod
    def _check_rows(t, x):
        B, H = x.shape[0], x.shape[2]
        if not t.is_cuda or t.device != x.device:
            raise L.FlairHipError("flair_amd.Unet: bottleneck rows must live on the input's HIP device")
        if tuple(t.shape) != (B, H // 32):
            raise RuntimeError(f"bottleneck rows must be (B, H/32) = ({B}, {H // 32}), got {tuple(t.shape)}")

    def _check_live(self, fwd_id):
        if fwd_id != self._live.id:
            raise RuntimeError("flair_amd.Unet: the activations of this forward were overwritten by a later training "
                               "forward; call backward before the next training-mode forward")

    def _new_grads(self):
        self._live.grads = torch.zeros(self._n_params, dtype=torch.float32, device=self._flat_p.device)
        return self._live.grads

    @_on_model_device
    def _c_backward(self, dlogits=None, dlogits_nhwc=None, grads=None, stage_events=None):
        ws = self._live.ws
        grads = grads if grads is not None else self._new_grads()
        ev = None
        if stage_events is not None:
            ev = (C.c_void_p * 7)(*[e.cuda_event for e in stage_events])
        L.check(L.lib().flair_unet_backward(self._h, L.ptr(self._flat_p), L.ptr(dlogits), L.ptr(dlogits_nhwc), L.ptr(grads),
                                            L.ptr(ws), ws.numel(), L.stream(), ev), "flair_unet_backward")
        self._live.rows = None
        return grads

    # ---- split path (model.py:57-62)
    @_on_model_device
    def _c_encoder_forward(self, x, training):
        x = self._prep(x)
        B, _, H, W = x.shape
        ws = self._workspace(B, H, W, training)
        chans = (64, 64, 128, 256, 512)
        feats = [torch.empty(B, c, H >> (i + 1), W >> (i + 1), dtype=torch.float32, device=x.device) for i, c in enumerate(chans)]
        arr = (C.c_void_p * 5)(*[f.data_ptr() for f in feats])
        if not training:
            self._eval.key = None   # the split path re-lays the eval arena: the fused forward's constants are gone
        L.check(L.lib().flair_unet_encoder_forward(self._hh(training), L.ptr(self._flat_p), L.ptr(self._flat_b), L.ptr(x), arr, B, H, W,
                                                   int(training), L.ptr(ws), ws.numel(), L.stream()), "encoder_forward")
        if training:
            self._eval.note_native_write()   # running statistics are about to change
            self._live = _LiveForward(self._live.id + 1, ws, (B, H, W))
            self._bump_bn(0, self._n_bn_encoder)
        else:
            self._eval_split = ((B, H, W), ws)
        return feats

    @_on_model_device
    def _c_decoder_forward(self, feats, training):
        (B, H, W), ws = (self._live.shape, self._live.ws) if training else self._eval_split
        feats = [f.detach().to(torch.float32).contiguous() for f in feats]
        out = torch.empty(B, 16, H, W, dtype=torch.float32, device=feats[0].device)
        arr = (C.c_void_p * 5)(*[f.data_ptr() for f in feats])
        if not training:
            self._eval.key = None
        L.check(L.lib().flair_unet_decoder_forward(self._hh(training), L.ptr(self._flat_p), L.ptr(self._flat_b), arr, L.ptr(out), B, H, W,
                                                   int(training), L.ptr(ws), ws.numel(), L.stream()), "decoder_forward")
        if training:
            self._eval.note_native_write()   # decoder running statistics changed
            self._bump_bn(self._n_bn_encoder)
        return out

    @_on_model_device
    def _c_head_forward(self, x, training):
        (B, H, W), ws = (self._live.shape, self._live.ws) if training else self._eval_split
        x = x.detach().to(torch.float32).contiguous()
        logits = torch.empty(B, self.classes, H, W, dtype=torch.float32, device=x.device)
        if not training:
            self._eval.key = None
        L.check(L.lib().flair_unet_head_forward(self._hh(training), L.ptr(self._flat_p), L.ptr(x), L.ptr(logits), B, H, W, int(training),
                                                L.ptr(ws), ws.numel(), L.stream()), "head_forward")
        return logits

    def _split_grads(self):
        return self._live.grads if self._live.grads is not None else self._new_grads()

    @_on_model_device
    def _c_head_backward(self, dlogits):
        (B, H, W), ws = self._live.shape, self._live.ws
        g = self._split_grads()
        dx = torch.empty(B, 16, H, W, dtype=torch.float32, device=dlogits.device)
        L.check(L.lib().flair_unet_head_backward(self._h, L.ptr(self._flat_p), L.ptr(dlogits), L.ptr(dx), L.ptr(g), L.ptr(ws),
                                                 ws.numel(), L.stream()), "head_backward")
        return dx

    @_on_model_device
    def _c_decoder_backward(self, dout):
        (B, H, W), ws = self._live.shape, self._live.ws
        g = self._split_grads()
        chans = (64, 64, 128, 256, 512)
        dfe = [torch.empty(B, c, H >> (i + 1), W >> (i + 1), dtype=torch.float32, device=dout.device) for i, c in enumerate(chans)]
        arr = (C.c_void_p * 5)(*[f.data_ptr() for f in dfe])
        L.check(L.lib().flair_unet_decoder_backward(self._h, L.ptr(self._flat_p), L.ptr(dout), arr, L.ptr(g), L.ptr(ws),
                                                    ws.numel(), L.stream()), "decoder_backward")
        return dfe

    @_on_model_device
    def _c_encoder_backward(self, dfeats):
        ws = self._live.ws
        g = self._split_grads()
        arr = (C.c_void_p * 5)(*[f.data_ptr() for f in dfeats])
        L.check(L.lib().flair_unet_encoder_backward(self._h, L.ptr(self._flat_p), arr, L.ptr(g), L.ptr(ws), ws.numel(),
                                                    L.stream()), "encoder_backward")

    # -------------------------------------------------------------------------------------------- nn.Module surface
    def _needs_graph(self):
        return torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters())

    def forward(self, x):
        if self._needs_graph():
            _, params = self._params_list()
            return _WholeFn.apply(self, x, *params)
        if torch.is_grad_enabled() and not self.training and any(p.requires_grad for p in self.parameters()):
            warnings.warn("flair_amd.Unet: eval-mode forward builds no autograd graph (wrap it in torch.no_grad())", stacklevel=2)
        return self._c_forward(x, training=self.training)

    def _encoder_forward(self, x):
        if self._needs_graph():
            _, params = self._params_list("encoder")
            feats = list(_EncoderFn.apply(self, x, *params))
        else:
            feats = self._c_encoder_forward(x, training=self.training)
        return [x] + feats

    def _decoder_forward(self, *features):
        feats = list(features[1:])
        if self._needs_graph():
            _, params = self._params_list("decoder")
            return _DecoderFn.apply(self, *feats, *params)
        return self._c_decoder_forward(feats, training=self.training)

    def _head_forward(self, x):
        if self._needs_graph():
            _, params = self._params_list("segmentation_head")
            return _HeadFn.apply(self, x, *params)
        return self._c_head_forward(x, training=self.training)

    @torch.no_grad()
    def predict(self, x):
        was = self.training
        self.eval()
        try:
            return self.forward(x)
        finally:
            self.train(was)

    @torch.no_grad()
    @_on_model_device
    def predict_classes(self, x, want_prob=False, bottleneck_rows=None, tta=None):
        """Eval-mode forward whose head convolution returns the argmax class per pixel (uint8 (B,H,W)) and, with ``want_prob``,
        that class's softmax probability (fp32 (B,H,W)) from its epilogue — what ``convert(softmax(model(x)), 'argmax')`` of
        zone_detect (dataset.py:23-30) and ``predict_step`` (task_module.py:206-213) compute — without writing the logits.
        ``bottleneck_rows``: fp32 (B, H/32), added to the bottleneck feature as ``feats[-1][b,c,h,w] += rows[b,h]`` (the
        metadata fusion of model.py:57-62) inside the same native call.
        ``tta`` (``flair_amd.tta.tta_codes``: "flips", "d4" or a list of transform codes): the mean probability over those D4
        transforms of ``x`` instead, from the fp32 logits of ``eval_logits`` (the rows go unchanged to every pass)."""
        if not x.is_cuda:
            raise L.FlairHipError("flair_amd.Unet needs HIP tensors (no CPU fallback)")
        codes = tta_codes(tta)
        if codes is not None:
            return tta_predict(lambda t: self.eval_logits(t, bottleneck_rows=bottleneck_rows), x, codes, want_prob=want_prob)
        B, H, W = x.shape[0], x.shape[-2], x.shape[-1]   # (_c_forward checks and prepares the input: once per call, it is host time)
        preds = torch.empty(B, H, W, dtype=torch.uint8, device=x.device)
        prob = torch.empty(B, H, W, dtype=torch.float32, device=x.device) if want_prob else None
        self._c_forward(x, training=False, want_logits=False, preds=preds, prob=prob, rows=bottleneck_rows)
        return (preds, prob) if want_prob else preds

    @torch.no_grad()
    def eval_logits(self, x, bottleneck_rows=None):
        """Eval-mode forward (running statistics, whatever ``self.training`` says) -> fp32 (B,classes,H,W) logits, with
        ``bottleneck_rows`` as for ``predict_classes``: encoder, metadata add, decoder and head of model.py:57-62 in one native
        call.  Builds no autograd graph."""
        return self._c_forward(x, training=False, rows=bottleneck_rows)

    def __del__(self):
        try:
            for k in ("_h", "_h_eval"):
                h = self.__dict__.get(k)
                if h:
                    L.lib().flair_unet_destroy(h)
        except Exception:
            pass

    def __getstate__(self):
        d = {k: v for k, v in self.__dict__.items() if k not in self._native_state}   # (the names _reset_native_state assigned)
        if self._flat_p is not None:
            # every parameter is a view of the flat buffer and pickle writes a view's WHOLE storage, once per tensor (some hundred
            # times 85 MB): hand out compact clones instead.  (The sub-modules' _owner, this object, is not copied along:
            # __setstate__ sets it.)
            d["_modules"] = copy.deepcopy(d["_modules"], {id(self): None})
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)
        self._reset_native_state()
        for m in (self.encoder, self.decoder, self.segmentation_head):
            object.__setattr__(m, "_owner", self)


def create_model(arch, encoder_name="resnet34", encoder_weights="imagenet", in_channels=3, classes=1, **kwargs):
    """``smp.create_model`` for the one architecture the reference instantiates (src/flair/model.py:37-41)."""
    archs = {"unet": Unet}
    try:
        cls = archs[arch.lower()]
    except KeyError:
        raise KeyError(f"Wrong architecture type `{arch}`. Available options are: {list(archs.keys())}")
    return cls(encoder_name=encoder_name, encoder_weights=encoder_weights, in_channels=in_channels, classes=classes, **kwargs)
