"""Objectives of the fused head beyond the reference's weighted cross entropy: label smoothing, a focal term and a soft Dice term
(the criteria the reference's model library ships as ``smp.losses``), computed by csrc/seg_loss.hip in the same pass that yields
the gradient, the argmax and the confusion matrix.

``SegLoss`` is a specification: hyper-parameters without tensors.  ``ops.seg_loss`` runs one on fp32 (B, C, H, W) logits,
``head.FusedSegLoss`` is the criterion object for the LightningModule surface, ``SegTrainer(..., loss=SegLoss(...))`` trains
with one.  Without a specification every path runs the reference's criterion (tasks_utils.py:88-93) through ``flair_ce_head``.

Definitions.  z are the logits, p = softmax(z) over the C classes, y_i the label of pixel i, v_i = 1 iff 0 <= y_i < C (every
label kind; all-zero one-hot pixels are class 0), w the class weights (ones when none are given), D = sum_i v_i w[y_i].

* CE term, focal_gamma == 0:   (1/D) sum_i v_i [(1 - e) w[y_i] (-log p_{i,y_i}) + (e/C) sum_c w[c] (-log p_ic)],  e = label_smoothing
  -- ``F.cross_entropy(z, y, weight=w, ignore_index, label_smoothing=e)`` with mean reduction.
* CE term, focal_gamma >= 1:   (1/D) sum_i v_i w[y_i] q_i^gamma (-log p_{i,y_i}),  q_i = sum over c != y_i of p_ic (summed from
  the other classes, never formed as 1 - p_y).  gamma -> 0 gives the weighted CE.  D == 0 behaves as the CE head does (0 / 0).
* Dice term (soft, multiclass; smp's ``DiceLoss`` with the ignored pixels masked).  A pixel counts iff k_i = v_i and w[y_i] > 0;
  I_c = sum k_i p_ic [y_i = c],  P_c = sum k_i p_ic,  T_c = sum k_i [y_i = c];
  Dice = (1/C) sum_c [T_c > 0] (1 - (2 I_c + s) / max(P_c + T_c + s, eps)),  s = dice_smooth, eps = dice_eps.
  The sums run over the batch of the call (under DDP each rank's own, as BatchNorm statistics).  No counted pixel: 0, gradient 0.
  Gradient: g_c = [T_c > 0]/C ((2 I_c + s)/(P_c + T_c + s)^2 - 2 [y_i = c]/(P_c + T_c + s)) where the clamp is not active,
  d Dice / d z_ik = k_i p_ik (g_k - sum_c g_c p_ic).
* loss = ce * CE + dice * Dice; the gradient has the mean reduction folded in, as ``flair_ce_head``'s.
"""
from __future__ import annotations

import math
import numbers

_FIELDS = ("ce", "label_smoothing", "focal_gamma", "dice", "dice_smooth", "dice_eps")


class SegLoss:
    """loss = ce * CE(label_smoothing | focal_gamma) + dice * Dice(dice_smooth, dice_eps); see the module docstring."""

    def __init__(self, ce=1.0, label_smoothing=0.0, focal_gamma=0.0, dice=0.0, dice_smooth=0.0, dice_eps=1e-7):
        vals = dict(ce=ce, label_smoothing=label_smoothing, focal_gamma=focal_gamma, dice=dice, dice_smooth=dice_smooth, dice_eps=dice_eps)
        for k, v in vals.items():
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
                raise ValueError(f"Invalid {k} value: {v!r} (a finite real number: int, float or a numpy scalar; not a string)")
        if ce < 0:
            raise ValueError(f"Invalid ce value: {ce} (the CE term's coefficient is >= 0)")
        if dice < 0:
            raise ValueError(f"Invalid dice value: {dice} (the Dice term's coefficient is >= 0)")
        if ce == 0 and dice == 0:
            raise ValueError("ce and dice are both 0: the loss has no term")
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"Invalid label_smoothing value: {label_smoothing} (in [0, 1))")
        if focal_gamma != 0 and focal_gamma < 1:
            raise ValueError(f"Invalid focal_gamma value: {focal_gamma} (0, or >= 1: below 1 the gradient is unbounded at p_y = 1)")
        if label_smoothing > 0 and focal_gamma > 0:
            raise ValueError("label_smoothing and focal_gamma exclude each other")
        if ce == 0 and label_smoothing > 0:
            raise ValueError("label_smoothing needs the CE term (ce > 0)")
        if ce == 0 and focal_gamma > 0:
            raise ValueError("focal_gamma needs the CE term (ce > 0)")
        if dice_smooth < 0:
            raise ValueError(f"Invalid dice_smooth value: {dice_smooth} (>= 0)")
        if dice_eps <= 0:
            raise ValueError(f"Invalid dice_eps value: {dice_eps} (> 0)")
        for k, v in vals.items():
            setattr(self, k, float(v))

    def astuple(self):
        """The six floats of ``flair_seg_loss_t``, in its order."""
        return tuple(getattr(self, k) for k in _FIELDS)

    def __eq__(self, other):
        return isinstance(other, SegLoss) and self.astuple() == other.astuple()

    def __hash__(self):
        return hash(self.astuple())

    def __repr__(self):
        return "SegLoss(" + ", ".join(f"{k}={getattr(self, k)}" for k in _FIELDS) + ")"


def from_config(config):
    """The specification of the config's optional ``loss: {ce:, label_smoothing:, focal_gamma:, dice:, dice_smooth:, dice_eps:}``
    key; without the key None: the reference's criterion."""
    entry = config.get("loss")
    if entry is None:
        return None
    if not isinstance(entry, dict):
        raise ValueError("config['loss'] must be a mapping (ce, label_smoothing, focal_gamma, dice, dice_smooth, dice_eps)")
    unknown = sorted(set(entry) - set(_FIELDS))
    if unknown:
        raise ValueError(f"unknown entries in config['loss']: {unknown} (known: {list(_FIELDS)})")
    return SegLoss(**entry)
