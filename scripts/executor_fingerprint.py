#!/usr/bin/env python3
"""What the U-Net executor (csrc/unet.hip) decides, as one JSON document for the build FLAIR_HIP_LIB names (default: the tree's).

    python scripts/executor_fingerprint.py [--out FILE] [--condensed]

Two builds whose documents are equal as text ran the same kernels the same number of times and left the same bits.  The document
holds no device name, path or time.

"plan": flair_unet_workspace_bytes over dtypes, shapes, training modes and class counts, and once per executor switch set to its
non-default.  The dry run walks the whole description logic, so a path decision that moves shows as a total that moves.  Needs no GPU.
"steps" (with a GPU): per configuration a fixed sequence of phases; per phase the {kernel name: launches} of the library's profile
and the SHA-256 of every tensor the phase leaves.  The two-step training phase again under each switch.
--condensed: per phase one SHA-256 over its launch table and one over its tensor hashes (the form profiles/ keeps)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flair-1_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import flair_amd  # noqa: E402
from flair_amd import _lib as L  # noqa: E402
from launch_helpers import profiled, tuned  # noqa: E402

_HDR = open(os.path.join(ROOT, "flair-1_amd", "csrc", "bwd_halo16.h")).read()
DEFAULTS = {"FLAIR_LAZY_BN": 1, "FLAIR_LAZY_HG": 1, "FLAIR_STEM_POOL": 1, "FLAIR_BNR_RES": 1, "FLAIR_BWD_FUSE": 1, "FLAIR_POOL_BNR": 1,
            "FLAIR_BWD16_FUSE": int(re.search(r"FLAIR_BWD16_FUSE_DEFAULT = (\d+)", _HDR).group(1)), "FLAIR_WGRAD_STREAM": 1, "FLAIR_WG_CUS": 0}
SWITCHES = [("FLAIR_LAZY_BN", 0), ("FLAIR_LAZY_BN", 2), ("FLAIR_LAZY_HG", 0), ("FLAIR_STEM_POOL", 0), ("FLAIR_BNR_RES", 0),
            ("FLAIR_BWD_FUSE", 0), ("FLAIR_POOL_BNR", 0), ("FLAIR_BWD16_FUSE", 0), ("FLAIR_BWD16_FUSE", 1), ("FLAIR_WGRAD_STREAM", 0),
            ("FLAIR_WG_CUS", 192)]
SHAPES = [(1, 32, 32), (2, 64, 64), (1, 96, 96), (4, 256, 512)]
DT = {"f32": 0, "bf16": 1}


def plan():
    out = {}
    handles = {}
    for dt, code in DT.items():
        for classes in (13, 19):
            h = C.c_void_p()
            L.check(L.lib().flair_unet_create(C.byref(h), 5, classes, code), "flair_unet_create")
            handles[dt, classes] = h
            for B, H, W in SHAPES:
                out[f"{dt} classes={classes} {B}x{H}x{W}"] = [L.lib().flair_unet_workspace_bytes(h, B, H, W, t) for t in (0, 1, 2)]
    for key, val in SWITCHES:
        with tuned([(key, val)], DEFAULTS):
            out[f"bf16 classes=13 2x64x64 {key}={val}"] = [L.lib().flair_unet_workspace_bytes(handles["bf16", 13], 2, 64, 64, t) for t in (0, 1, 2)]
    for h in handles.values():
        L.lib().flair_unet_destroy(h)
    return out


def sha(t):
    if isinstance(t, (list, tuple)):
        return [sha(v) for v in t]
    return hashlib.sha256(t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def phase(fn):
    left, ran = profiled(fn, slots=2048)
    torch.cuda.synchronize()
    return {"launches": ran, "sha256": {k: sha(v) for k, v in left.items()}}


def fresh(state, classes, dtype, dev):
    m = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=classes, compute_dtype=dtype)
    m.load_state_dict(state, strict=True)
    return m.to(dev).train()


def batch(g, shape, classes, dev):
    x = torch.randn(*shape, generator=g).to(dev)
    lab = torch.randint(0, classes, (shape[0], shape[2], shape[3]), generator=g)
    return x, lab.to(dev)


def train2(state, classes, shape, dtype, dev):
    """two SegTrainer.train_steps of a fresh model, as tests/test_gpu_bwd16_fuse.py::_steps takes them"""
    m = fresh(state, classes, dtype, dev)
    tr = flair_amd.SegTrainer(m, lr=0.05, class_weight=torch.linspace(0.5, 2, classes))
    g = torch.Generator().manual_seed(shape[2])

    def run():
        left = {"loss": [], "grads": []}
        for _ in range(2):
            x, lab = batch(g, shape, classes, dev)
            left["loss"].append(tr.train_step(x, lab.to(torch.uint8)).clone())
            left["grads"].append(tr.grads.clone())
        left.update(params=m.flat_parameters(), buffers=m.flat_buffers(), confmat=tr.confmat)
        return left

    return phase(run), m, tr, g


def autograd_step(m, forward, x, lab):
    for p in m.parameters():
        p.grad = None
    logits = forward(x)
    loss = torch.nn.functional.cross_entropy(logits, lab)
    loss.backward()
    return {"logits": logits, "loss": loss, "grads": [p.grad for p in m.parameters()], "buffers": m.flat_buffers()}


def config(state, classes, shape, dtype, dev):
    out = {}
    out["train_step x2"], m, tr, g = train2(state, classes, shape, dtype, dev)
    B, _, H, W = shape
    x, lab = batch(g, shape, classes, dev)
    rows = torch.randn(B, H // 32, generator=g).to(dev)
    out["autograd model(x)"] = phase(lambda: autograd_step(m, m, x, lab))
    out["autograd split path"] = phase(lambda: autograd_step(m, lambda t: m.segmentation_head(m.decoder(*m.encoder(t))), x, lab))

    def rows_step():
        drows = torch.full((B, H // 32), float("nan"), device=dev)
        logits = m._c_forward(x, training=True, train_rows=(rows, drows))
        onehot = torch.nn.functional.one_hot(lab, classes).permute(0, 3, 1, 2).float()
        dl = ((torch.softmax(logits, dim=1) - onehot) / lab.numel()).contiguous()
        grads = m._c_backward(dlogits=dl, grads=torch.zeros_like(m.flat_parameters()))
        return {"logits": logits, "grads": grads, "drows": drows, "buffers": m.flat_buffers()}

    out["training step with train_rows"] = phase(rows_step)
    out["eval_logits"] = phase(lambda: {"logits": m.eval_logits(x)})
    out["eval_logits bottleneck_rows"] = phase(lambda: {"logits": m.eval_logits(x, bottleneck_rows=rows)})
    out["predict_classes want_prob"] = phase(lambda: dict(zip(("preds", "prob"), m.predict_classes(x, want_prob=True))))
    out["validate_step"] = phase(lambda: {"loss": tr.validate_step(x, lab.to(torch.uint8)).clone(), "confmat": tr.val_confmat,
                                          "preds": tr._val_preds})
    return out


def steps():
    from oracle import unet_resnet34 as om
    dev = torch.device("cuda:0")
    states = {c: om.seeded_model(5, c, 31).state_dict() for c in (13, 19)}
    out = {}
    for dtype, shape, classes in (("bf16", (2, 5, 64, 64), 13), ("bf16", (1, 5, 96, 96), 13), ("f32", (2, 5, 64, 64), 13),
                                  ("bf16", (2, 5, 64, 64), 19)):
        out[f"{dtype} classes={classes} {'x'.join(map(str, shape))}"] = config(states[classes], classes, shape, dtype, dev)
    for key, val in SWITCHES:
        with tuned([(key, val)], DEFAULTS):
            out[f"bf16 classes=13 2x5x64x64 train_step x2 {key}={val}"] = train2(states[13], 13, (2, 5, 64, 64), "bf16", dev)[0]
    return out


def condensed(doc):
    digest = lambda v: hashlib.sha256(json.dumps(v, sort_keys=True).encode()).hexdigest()
    out = {"plan": doc["plan"]}
    for name, c in doc.get("steps", {}).items():
        for ph, p in ({name: c} if "launches" in c else {f"{name}: {k}": v for k, v in c.items()}).items():
            out.setdefault("steps", {})[ph] = {"launches": sum(p["launches"].values()), "launches_sha256": digest(p["launches"]),
                                               "tensors_sha256": digest(p["sha256"])}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--condensed", action="store_true")
    args = ap.parse_args()
    doc = {"plan": plan()}
    if torch.cuda.is_available():
        doc["steps"] = steps()
    if args.condensed:
        doc = condensed(doc)
    text = json.dumps(doc, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
