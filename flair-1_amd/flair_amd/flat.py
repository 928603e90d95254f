"""Tensors as views of one flat fp32 buffer: the copy-and-rebind of ``Unet.flatten_``, ``NativeModel._flatten`` and the fused
trainer's MetadataMLP binding, and the check that such a binding still stands.  Pure torch, any device."""
from __future__ import annotations

import math

import torch


def aliased(flat, items):
    """``items``: (tensor, float offset) pairs.  True when every tensor is fp32, on ``flat``'s device and starts at its offset of
    ``flat`` — what ``.data =`` rebinds, ``.to()`` / ``.double()`` and ``load_state_dict(assign=True)`` undo."""
    if flat is None:
        return False
    base = flat.data_ptr()
    return all(t.dtype == torch.float32 and t.device == flat.device and t.data_ptr() == base + 4 * off for t, off in items)


def bind(items, n, device):
    """``items``: (tensor, float offset, shape) triples.  A new zero-filled flat buffer of ``n`` floats on ``device`` with every
    tensor's values copied to its offset and the tensor rebound as a ``.data`` view of that slot.  One ``copy_`` per tensor: the new
    buffer's version counter is the number of tensors, and ``.data =`` moves no counter."""
    flat = torch.zeros(n, dtype=torch.float32, device=device)
    with torch.no_grad():
        for t, off, shape in items:
            view = flat[off:off + math.prod(shape)].view(shape)
            view.copy_(t.detach().to(device=device, dtype=torch.float32))
            t.data = view
    return flat
