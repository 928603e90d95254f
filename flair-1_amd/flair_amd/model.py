"""Mirror of /root/reference/src/flair/model.py (``FLAIR_ModelFactory`` :7-70, ``MetadataMLP`` :74-96).

Same constructor argument (the YAML config dict), same attributes (``seg_model``, ``enc``) and the same
``forward(x, met=None)``.  Differences, all documented in DESIGN.md:
  * ``smp.create_model`` is served by ``flair_amd.unet.create_model`` (the HIP executor);
  * the reference's ``NameError`` at model.py:32 (bare ``model_provider``) is fixed to ``self.model_provider``;
  * the metadata broadcast ``x_enc.unsqueeze(1).unsqueeze(-1).repeat(1,512,1,16)`` + ``torch.add``
    (model.py:59-60; element [b,c,h,w] += x_enc[b,h]) runs as one in-place HIP kernel on a copy of feats[-1]
    instead of materialising the (B,512,16,16) repeat; with an eval-mode ``seg_model`` the add happens inside ONE native forward
    (``Unet.eval_logits(x, bottleneck_rows=x_enc)``, rows_f32 of flair_unet_fwd_opts_t) on the executor's own NHWC bottleneck — no fp32 NCHW
    round trip of the features, constants reused, HIP-graph replay at small batches; FLAIR_META_FUSE=0 (read per call) keeps the
    three-call split path, which a training-mode ``seg_model`` always takes;
  * the HuggingFace provider branch (model.py:43-50,66-68) builds SegFormer-MiT and 3-channel UperNet-Swin natively
    (inference only); other names raise.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .tta import tta_codes, tta_predict
from .unet import create_model


def check_metadata_tile(x):
    """The reference hard-codes repeat(1,512,1,16) (model.py:59, quirk Q4): the metadata branch takes 512 x 512 tiles only."""
    if tuple(x.shape[-2:]) != (512, 512):
        raise RuntimeError("metadata fusion expects a (B,512,16,16) bottleneck (512x512 input tiles)")


class _AddRowVec(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, x_enc):
        out = feat.detach().clone().contiguous()
        N, C, H, W = out.shape
        L.check(L.lib().flair_add_rowvec_nchw(L.ptr(out), L.ptr(x_enc.detach().float().contiguous()), N, C, H, W, L.stream()))
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g.sum(dim=(1, 3))


def _ptr3(ts):
    import ctypes as C
    return (C.c_void_p * 3)(*[None if t is None else L.ptr(t) for t in ts])


class _MlpFn(torch.autograd.Function):
    """The three Linear + Dropout + ReLU layers as ONE HIP kernel each way (flair_metadata_mlp_forward / _backward)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, masks):
        x = x.detach().float().contiguous()
        B = x.shape[0]
        ws = [w.detach().float().contiguous() for w in (w1, w2, w3)]
        bs = [b.detach().float().contiguous() for b in (b1, b2, b3)]
        h1 = torch.empty(B, 64, dtype=torch.float32, device=x.device)
        h2 = torch.empty(B, 32, dtype=torch.float32, device=x.device)
        out = torch.empty(B, 16, dtype=torch.float32, device=x.device)
        L.check(L.lib().flair_metadata_mlp_forward(L.ptr(x), _ptr3(ws), _ptr3(bs), None if masks is None else _ptr3(masks),
                                                   L.ptr(h1), L.ptr(h2), L.ptr(out), B, L.stream()), "metadata_mlp_forward")
        ctx.save_for_backward(x, h1, h2, out, *ws)
        ctx.masks = masks
        return out

    @staticmethod
    def backward(ctx, g):
        x, h1, h2, out, w1, w2, w3 = ctx.saved_tensors
        B = x.shape[0]
        dw = [torch.empty_like(w) for w in (w1, w2, w3)]
        db = [torch.empty(n, dtype=torch.float32, device=x.device) for n in (64, 32, 16)]
        scratch = torch.empty(B * 112, dtype=torch.float32, device=x.device)
        L.check(L.lib().flair_metadata_mlp_backward(L.ptr(x), L.ptr(h1), L.ptr(h2), L.ptr(out), _ptr3([w1, w2, w3]),
                                                    None if ctx.masks is None else _ptr3(ctx.masks),
                                                    L.ptr(g.detach().float().contiguous()), B, _ptr3(dw), _ptr3(db),
                                                    L.ptr(scratch), L.stream()), "metadata_mlp_backward")
        return None, dw[0], db[0], dw[1], db[1], dw[2], db[2], None


class MetadataMLP(nn.Module):
    """Light MLP to encode metadata (model.py:74-96): 45 -> 64 -> 32 -> 16, Dropout(0.4) + ReLU each.  Same module tree
    and state_dict keys (enc_mlp.0 / .3 / .6) as the reference; on a HIP device the forward and backward are one kernel
    each (csrc/metadata_mlp.hip), with the dropout masks drawn here from torch's generator in training mode.  Host
    tensors (the CPU-side unit tests of the mirror) take the plain nn.Sequential."""

    def __init__(self):
        super().__init__()
        self.enc_mlp = nn.Sequential(
            nn.Linear(45, 64), nn.Dropout(0.4), nn.ReLU(),
            nn.Linear(64, 32), nn.Dropout(0.4), nn.ReLU(),
            nn.Linear(32, 16), nn.Dropout(0.4), nn.ReLU(),
        )

    def dropout_masks(self, B, device):
        """Bernoulli(keep = 0.6) / 0.6 per layer, as nn.Dropout(0.4) applies them; None in eval mode."""
        if not self.training:
            return None
        return [torch.bernoulli(torch.full((B, n), 0.6, device=device)) / 0.6 for n in (64, 32, 16)]

    def forward(self, x, masks="auto"):
        if not x.is_cuda:
            return self.enc_mlp(x)
        if x.dim() != 2 or x.shape[1] != 45:
            raise ValueError("MetadataMLP expects (B, 45) metadata vectors")
        if masks == "auto":
            masks = self.dropout_masks(x.shape[0], x.device)
        if x.shape[0] > 256:   # the backward kernel takes up to 256 samples per launch: larger batches go in slices
            parts = [self.forward(x[i:i + 256], None if masks is None else [m[i:i + 256] for m in masks])
                     for i in range(0, x.shape[0], 256)]
            return torch.cat(parts, 0)
        l1, l2, l3 = self.enc_mlp[0], self.enc_mlp[3], self.enc_mlp[6]
        return _MlpFn.apply(x, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias, masks)


class FLAIR_ModelFactory(nn.Module):
    def __init__(self, config, compute_dtype=None):
        super().__init__()
        self.model_provider = config["model_framework"]["model_provider"]
        self.use_metadata = config["use_metadata"]
        n_channels = int(len(config["channels"]))
        n_classes = int(len(config["classes"]))
        if self.use_metadata and self.model_provider == "SegmentationModelsPytorch":
            self.enc = MetadataMLP()
        if self.model_provider == "SegmentationModelsPytorch":
            encoder, architecture = config["model_framework"]["SegmentationModelsPytorch"]["encoder_decoder"].split("_")
            kw = {} if compute_dtype is None else {"compute_dtype": compute_dtype}
            if "encoder_weights" in config.get("model_framework", {}).get("SegmentationModelsPytorch", {}):
                kw["encoder_weights"] = config["model_framework"]["SegmentationModelsPytorch"]["encoder_weights"]
            self.seg_model = create_model(arch=architecture, encoder_name=encoder, classes=n_classes,
                                          in_channels=n_channels, **kw)
        elif self.model_provider == "HuggingFace":
            # model.py:43-50: AutoModelForSemanticSegmentation.from_pretrained(org_model, num_labels=...).  No hub here: the
            # SegFormer family (BASELINE config 5) and UperNet-Swin-tiny / -small are built natively from their published
            # geometry, weights arrive through load_state_dict; anything else raises.  Inference only.
            from .segformer import SegformerForSemanticSegmentation, config_for
            from .upernet import UperNetForSemanticSegmentation, config_for_upernet
            hf = config["model_framework"]["HuggingFace"]
            if "upernet" in hf["org_model"].lower():
                # UperNet-Swin (the provider's default, openmmlab/upernet-swin-small): the reference builds it from the hub config,
                # whose backbone takes 3 input channels, and never passes num_channels (quirk Q11) — any other band count fails in
                # its first forward.  Built here for exactly that case.
                kw = config_for_upernet(hf["org_model"])
                if n_channels != 3:
                    raise NotImplementedError(
                        f"{hf['org_model']!r} with {n_channels} channels: the reference builds this model with the hub config's 3 "
                        "input channels; build flair_amd.UperNetForSemanticSegmentation(num_channels=...) directly for other band counts")
                self.seg_model = UperNetForSemanticSegmentation(num_channels=3, num_labels=n_classes, compute_dtype=compute_dtype, **kw)
            else:
                kw = config_for(hf["org_model"])
                kw.update({k: hf[k] for k in ("depths", "decoder_hidden_size") if k in hf})
                self.seg_model = SegformerForSemanticSegmentation(num_channels=n_channels, num_labels=n_classes,
                                                                  compute_dtype=compute_dtype, **kw)

    def _meta_fused(self):
        """Metadata branch of an eval-mode U-Net: the add rides inside the single native forward (FLAIR_META_FUSE=0: split path)."""
        return not self.seg_model.training and os.environ.get("FLAIR_META_FUSE", "1") != "0"

    def forward(self, x, met=None):
        if self.use_metadata == True and self.model_provider == "SegmentationModelsPytorch":  # noqa: E712
            if self._meta_fused():
                x_enc = self.enc(met)
                check_metadata_tile(x)
                return self.seg_model.eval_logits(x, bottleneck_rows=x_enc)
            feats = self.seg_model.encoder(x)
            x_enc = self.enc(met)
            check_metadata_tile(x)   # (behind the encoder: a tile it refuses raises its own error first)
            feats[-1] = _AddRowVec.apply(feats[-1], x_enc)
            output = self.seg_model.decoder(*feats)
            output = self.seg_model.segmentation_head(output)
        elif self.model_provider == "HuggingFace":
            output = self.seg_model(x).logits   # model.py:66-68
        else:
            output = self.seg_model(x)
        return output

    @torch.no_grad()
    def predict_classes(self, x, met=None, want_prob=False, tta=None):
        """argmax(softmax(forward(x, met))) as uint8 (B,H,W) and, with ``want_prob``, the winner's fp32 probability — what
        ``predict_step`` (task_module.py:206-213) and zone_detect's 'argmax' output compute.  The U-Net takes both out of its head
        convolution's epilogue (``Unet.predict_classes``), with metadata through the same single native call; the MetadataMLP
        runs without dropout, as Lightning's ``model.eval()`` makes the reference's.  Other models: the separate kernel over
        the logits.
        ``tta`` ("flips", "d4" or a list of D4 transform codes, ``flair_amd.tta``): the mean probability over those transforms of
        ``x`` instead, at the resolution of this model's logits (a SegFormer's stay quarter-size, quirk Q11); the metadata vectors go
        unchanged to every pass."""
        codes = tta_codes(tta)
        if self.model_provider == "SegmentationModelsPytorch":
            if self.use_metadata != True:  # noqa: E712
                return self.seg_model.predict_classes(x, want_prob=want_prob, tta=codes)
            if met is None:
                raise ValueError("this model was built with use_metadata: predict_classes needs the (B,45) metadata vectors")
            if os.environ.get("FLAIR_META_FUSE", "1") != "0":
                x_enc = self.enc(met, masks=None)
                check_metadata_tile(x)
                return self.seg_model.predict_classes(x, want_prob=want_prob, bottleneck_rows=x_enc, tta=codes)
        if codes is not None:
            return tta_predict(lambda t: self.forward(t, met), x, codes, want_prob=want_prob)
        logits = self.forward(x, met)
        return ops.softmax_argmax(logits.detach().float().contiguous(), want="u8", want_maxprob=want_prob)
