"""Host-side mirror of ``transformers.SegformerForSemanticSegmentation`` (inference) over the HIP executor.

The reference's zone_detect builds its HuggingFace model with ``AutoModelForSemanticSegmentation.from_pretrained``
(/root/reference/src/zone_detect/model.py:42-50, src/flair/model.py:43-50) and runs ``model(imgs).logits``
(compare.py:31-36, model.py:66-68); BASELINE config 5 names SegFormer-MiT-B2 with 5 input channels.  This module is that
object by interface: ``forward(pixel_values) -> output.logits`` of shape (B, num_labels, H/4, W/4), ``state_dict()`` /
``load_state_dict()`` with the library's key names and shapes (transformers 5.x: ``segformer.stages.<i>...``,
``decode_head...``), ``eval()`` only.  ``forward_full`` additionally returns the logits after the x4 bilinear upsample
(align_corners=False) that softmax / margin crop / convert need at tile resolution (the library's own loss path does the
same interpolation).

The nn.Module tree below holds PARAMETER CONTAINERS only; all arithmetic runs in libflair_hip.so
(flair_segformer_forward), host tensors are refused.  Every tensor is a view of one flat fp32 device buffer laid out by the
native tensor table.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from types import SimpleNamespace

import torch

from . import _lib as L
from ._native_model import NativeModel

# published MiT geometries (SegFormer paper, table 6): depths per stage; hidden sizes 64/128/320/512, heads 1/2/5/8 and
# reduction ratios 8/4/2/1 are common to B1 .. B5; decode-head width 256 for B1, 768 from B2 on
MIT_DEPTHS = {"b1": (2, 2, 2, 2), "b2": (3, 4, 6, 3), "b3": (3, 4, 18, 3), "b4": (3, 8, 27, 3), "b5": (3, 6, 40, 3)}


def config_for(org_model: str) -> dict:
    """'nvidia/mit-b2', 'nvidia/segformer-b2-finetuned-...' -> constructor keywords (no hub access here: geometry only)."""
    m = re.search(r"(?:mit|segformer)[-_]?(b[1-5])", org_model.lower())
    if not m:
        raise NotImplementedError(f"HuggingFace model {org_model!r}: only SegFormer / MiT-B1..B5 are built natively")
    v = m.group(1)
    return {"depths": MIT_DEPTHS[v], "decoder_hidden_size": 256 if v == "b1" else 768}


class SegformerForSemanticSegmentation(NativeModel):
    _PREFIX = "segformer"
    _BAD_TILE = ("unsupported tile size {H}x{W}: H and W must be multiples of 32 with (H/32)*(W/32) a "
                 "multiple of 16 and at most 256 (e.g. 128, 256, 512)")

    def __init__(self, num_channels=3, num_labels=150, depths=(3, 4, 6, 3), hidden_sizes=(64, 128, 320, 512),
                 num_attention_heads=(1, 2, 5, 8), sr_ratios=(8, 4, 2, 1), decoder_hidden_size=768, compute_dtype=None,
                 initializer_range=0.02):
        super().__init__()
        self._dt = L.dtype_code(compute_dtype if compute_dtype is not None else os.environ.get("FLAIR_AMD_DTYPE", "f32"))
        self.num_channels, self.num_labels = int(num_channels), int(num_labels)
        self.config = SimpleNamespace(num_channels=self.num_channels, num_labels=self.num_labels, depths=tuple(depths),
                                      hidden_sizes=tuple(hidden_sizes), num_attention_heads=tuple(num_attention_heads),
                                      sr_ratios=tuple(sr_ratios), decoder_hidden_size=int(decoder_hidden_size))
        arr = lambda v: (C.c_int * 4)(*[int(x) for x in v])
        h = C.c_void_p()
        L.check(L.lib().flair_segformer_create(C.byref(h), self.num_channels, self.num_labels, arr(depths), arr(hidden_sizes),
                                               arr(num_attention_heads), arr(sr_ratios), int(decoder_hidden_size), self._dt),
                "flair_segformer_create")
        self._init_tensors(h, initializer_range)
        self.eval()

    def _run(self, x, want_quarter, want_full):
        flat, x = self._prepare(x)
        B, _, H, W = x.shape
        with torch.cuda.device(flat.device):
            lq = torch.empty(B, self.num_labels, H // 4, W // 4, dtype=torch.float32, device=x.device) if want_quarter else None
            lf = torch.empty(B, self.num_labels, H, W, dtype=torch.float32, device=x.device) if want_full else None
            L.check(L.lib().flair_segformer_forward(self._h, L.ptr(flat), L.ptr(x), L.ptr(lq), L.ptr(lf), B, H, W, L.ptr(self._ws),
                                                    self._ws.numel(), L.stream()), "flair_segformer_forward")
        return lq, lf

    @torch.no_grad()
    def forward(self, pixel_values, labels=None, **_):
        if labels is not None:
            raise RuntimeError("inference-only: no loss")
        lq, _ = self._run(pixel_values, True, False)
        return SimpleNamespace(logits=lq, loss=None)

    @torch.no_grad()
    def forward_full(self, pixel_values):
        """logits after nn.functional.interpolate(size=input size, mode='bilinear', align_corners=False): (B, labels, H, W)"""
        return self._run(pixel_values, False, True)[1]

    @torch.no_grad()
    def forward_quarter(self, pixel_values):
        """the decode head's own output, (B, labels, H/4, W/4) fp32 — the same tensor as ``forward(x).logits`` — for the
        zone_detect consumers of quarter-resolution logits (``detect_convert(..., upsample=4)``)"""
        return self._run(pixel_values, True, False)[0]
