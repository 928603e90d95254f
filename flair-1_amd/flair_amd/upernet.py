"""Host-side mirror of ``transformers.UperNetForSemanticSegmentation`` with a ``SwinBackbone`` (inference) over the HIP executor.

The reference's HuggingFace provider defaults to ``openmmlab/upernet-swin-small`` in every config it ships, and its zone_detect
runs ``model(imgs).logits``.  This module is that object by interface: ``forward(pixel_values) -> output.logits`` of shape
(B, num_labels, H, W) — UperNet resizes its logits to the input size itself — and ``state_dict()`` / ``load_state_dict()`` with the
library's key names, order and shapes (transformers 5.x: ``backbone.swin...``, ``backbone.hidden_states_norms...``,
``decode_head...``, ``auxiliary_head...``), ``eval()`` only.  ``load_state_dict`` also takes the transformers-4.x names every
checkpoint of the reference carries (its pin is transformers <= 4.50.3), renamed by the table below.  The auxiliary head loads and
is never computed.

The nn.Module tree holds PARAMETER CONTAINERS only; all arithmetic runs in libflair_hip.so (flair_upernet_forward), host tensors
are refused.  Every tensor is a view of one flat fp32 device buffer laid out by the native tensor table.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from types import SimpleNamespace

import torch

from . import _lib as L
from ._native_model import NativeModel

# published geometries: embed_dim 96, heads 3 / 6 / 12 / 24, window 7 for both; only the depth of stage 3 differs
UPERNET_SWIN_DEPTHS = {"tiny": (2, 2, 6, 2), "small": (2, 2, 18, 2)}

# transformers 4.x -> 5.x names of the Swin backbone (the library's own "swin" / "SwinBackbone" conversion mapping), applied in
# this order: `attention.output.dense` before the bare `output.dense`
LEGACY_RENAMES = (
    (r"attention\.self\.query\.", "attention.q_proj."),
    (r"attention\.self\.key\.", "attention.k_proj."),
    (r"attention\.self\.value\.", "attention.v_proj."),
    (r"attention\.self\.relative_position_bias_table", "attention.relative_position_bias.relative_position_bias_table"),
    (r"attention\.output\.dense\.", "attention.o_proj."),
    (r"intermediate\.dense\.", "mlp.fc1."),
    (r"(?<![a-z_])output\.dense\.", "mlp.fc2."),
    (r"^backbone\.embeddings\.", "backbone.swin.embeddings."),
    (r"^backbone\.encoder\.", "backbone.swin.encoder."),
)
# 4.x buffers that 5.x recomputes (non-persistent): dropped
LEGACY_DROPPED = re.compile(r"relative_position_index$")


def rename_legacy_keys(state_dict):
    """A state dict with transformers-4.x Swin names -> the 5.x names (other keys unchanged, ``relative_position_index`` dropped)."""
    out = type(state_dict)() if isinstance(state_dict, dict) else {}
    for k, v in state_dict.items():
        if LEGACY_DROPPED.search(k):
            continue
        for pat, rep in LEGACY_RENAMES:
            k = re.sub(pat, rep, k)
        out[k] = v
    return out


def config_for_upernet(org_model: str) -> dict:
    """'openmmlab/upernet-swin-small' / '-tiny' -> constructor keywords (no hub access here: geometry only)."""
    m = re.search(r"upernet[-_]swin[-_](tiny|small)\b", org_model.lower())
    if not m:
        raise NotImplementedError(f"HuggingFace model {org_model!r}: only UperNet with Swin-tiny / Swin-small is built natively")
    return {"depths": UPERNET_SWIN_DEPTHS[m.group(1)]}


class UperNetForSemanticSegmentation(NativeModel):
    _PREFIX = "upernet"
    _ZERO_LEAVES = ("bias", "relative_position_bias_table")
    _BAD_TILE = "unsupported tile size {H}x{W}: H and W must be multiples of 32 from 64 to 2048"

    def __init__(self, num_channels=3, num_labels=150, embed_dim=96, depths=(2, 2, 18, 2), num_heads=(3, 6, 12, 24), window_size=7,
                 hidden_size=512, pool_scales=(1, 2, 3, 6), auxiliary_in_channels=384, auxiliary_channels=256, compute_dtype=None,
                 initializer_range=0.02):
        super().__init__()
        self._dt = L.dtype_code(compute_dtype if compute_dtype is not None else os.environ.get("FLAIR_AMD_DTYPE", "f32"))
        self.num_channels, self.num_labels = int(num_channels), int(num_labels)
        if int(window_size) != 7:
            raise ValueError(f"window_size {window_size}: the native Swin attention is built for 7 x 7 windows (swin-tiny / -small)")
        if len(depths) != 4 or len(num_heads) != 4 or len(pool_scales) != 4:
            raise ValueError("four stages and four pool scales expected")
        self.config = SimpleNamespace(num_channels=self.num_channels, num_labels=self.num_labels, embed_dim=int(embed_dim),
                                      depths=tuple(depths), num_heads=tuple(num_heads), window_size=int(window_size),
                                      hidden_size=int(hidden_size), pool_scales=tuple(pool_scales),
                                      auxiliary_in_channels=int(auxiliary_in_channels), auxiliary_channels=int(auxiliary_channels))
        arr = lambda v: (C.c_int * 4)(*[int(x) for x in v])
        h = C.c_void_p()
        L.check(L.lib().flair_upernet_create(C.byref(h), self.num_channels, self.num_labels, int(embed_dim), arr(depths), arr(num_heads),
                                             int(window_size), int(hidden_size), arr(pool_scales), int(auxiliary_in_channels),
                                             int(auxiliary_channels), self._dt), "flair_upernet_create")
        self._init_tensors(h, initializer_range)
        self.eval()

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """The library's 5.x keys, or the 4.x keys of the reference's checkpoints (``rename_legacy_keys``).  A 4.x SwinBackbone has
        no ``layernorm`` (5.x wraps a whole SwinModel, whose final norm the backbone's outputs never pass through): a 4.x state dict
        leaves that norm as it is."""
        sd = rename_legacy_keys(state_dict)
        if any(k.startswith(("backbone.embeddings.", "backbone.encoder.")) for k in state_dict):
            own = self.state_dict()
            for k in ("backbone.swin.layernorm.weight", "backbone.swin.layernorm.bias"):
                if k not in sd:
                    sd[k] = own[k].detach().clone()
        return super().load_state_dict(sd, strict=strict, assign=assign)

    @torch.no_grad()
    def forward(self, pixel_values, labels=None, **_):
        if labels is not None:
            raise RuntimeError("inference-only: no loss")
        return SimpleNamespace(logits=self.forward_full(pixel_values), loss=None)

    @torch.no_grad()
    def forward_full(self, pixel_values):
        """the logits at the input size, (B, labels, H, W) — the same tensor as ``forward(x).logits``"""
        flat, x = self._prepare(pixel_values)
        B, _, H, W = x.shape
        with torch.cuda.device(flat.device):
            out = torch.empty(B, self.num_labels, H, W, dtype=torch.float32, device=x.device)
            L.check(L.lib().flair_upernet_forward(self._h, L.ptr(flat), L.ptr(x), L.ptr(out), B, H, W, L.ptr(self._ws), self._ws.numel(),
                                                  L.stream()), "flair_upernet_forward")
        return out

    @torch.no_grad()
    def forward_quarter(self, pixel_values):
        """the classifier's own output, (B, labels, H/4, W/4) fp32: ``forward_full`` is its x4 bilinear resize, which the
        zone_detect consumers of quarter-resolution logits apply per pixel instead (``detect_convert(..., upsample=4)``)"""
        flat, x = self._prepare(pixel_values)
        B, _, H, W = x.shape
        with torch.cuda.device(flat.device):
            out = torch.empty(B, self.num_labels, H // 4, W // 4, dtype=torch.float32, device=x.device)
            L.check(L.lib().flair_upernet_forward_quarter(self._h, L.ptr(flat), L.ptr(x), L.ptr(out), B, H, W, L.ptr(self._ws),
                                                          self._ws.numel(), L.stream()), "flair_upernet_forward_quarter")
        return out
