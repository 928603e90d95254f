"""Fused training step + data-parallel gradient exchange for the segmentation hot path.

One step = what Lightning drives per batch in the reference:
``training_step`` (src/flair/task_module.py:82-86: forward, CE, argmax, Jaccard update) ->
``loss.backward()`` -> DDP gradient all-reduce (src/flair/tasks.py:83-88, strategy 'ddp') ->
``SGD.step()`` (src/flair/tasks_utils.py:95).  Here every device-side piece is a HIP kernel behind the
C ABI and the exchange is RCCL over xGMI: one process per GPU, gradients live in ONE flat buffer laid
out stage by stage, the native backward records a HIP event when a stage's bucket is final, and the
bucket's all-reduce starts on a side stream while the earlier stages are still being differentiated.
BatchNorm batch statistics stay per rank (no SyncBN), like the reference; the RUNNING statistics are rank 0's on every
rank, like torch DDP's ``broadcast_buffers=True`` (the default Lightning's 'ddp' strategy keeps) leaves them: DDP sends rank
0's buffers to every rank in front of each forward, which for BatchNorm is the same as sending them behind each training
step — done here with one small broadcast per step on the exchange stream — so validation, predict, ``state_dict()`` and
checkpoints see rank 0's statistics on every rank without a collective of their own.
"""
from __future__ import annotations

import ctypes
import os

import torch
import torch.distributed as dist

from . import _lib as L
from . import flat as _flat
from . import losses as _losses
from . import ops
from . import optim as _optim
from .model import check_metadata_tile
from .tta import tta_codes


def bucket_ranges(stage_ranges, min_elems=0):
    """Gradient buckets in READY order (head first).  Small neighbours are merged so that no bucket is
    below ``min_elems`` floats: xGMI rings are per-link bound, tiny collectives only add latency."""
    out = []
    cur = None
    for b, e in reversed(list(stage_ranges)):
        if e <= b:
            continue
        cur = (b, e) if cur is None else (b, cur[1])
        if cur[1] - cur[0] >= min_elems:
            out.append(cur)
            cur = None
    if cur is not None:
        if out:
            out[-1] = (cur[0], out[-1][1])
        else:
            out.append(cur)
    return out


def allreduce_buckets(flat_grads, buckets, group=None, async_op=False):
    """Sum-all-reduce each bucket view of the flat gradient buffer (works on gloo/CPU for tests)."""
    works = []
    for b, e in buckets:
        w = dist.all_reduce(flat_grads[b:e], op=dist.ReduceOp.SUM, group=group, async_op=async_op)
        if async_op:
            works.append(w)
    return works


def reduce_validation_state(loss_sum, count, confmat, group=None):
    """Sum the validation accumulators over the ranks, in place: what ``sync_dist=True`` / torchmetrics'
    ``dist_reduce_fx="sum"`` do to MeanMetric's (value, weight) and to the confusion matrix of MulticlassJaccardIndex
    (task_module.py:111-135).  Plain torch.distributed on whatever device the tensors live on."""
    lc = torch.stack([loss_sum, count.to(loss_sum.dtype)])
    dist.all_reduce(lc, op=dist.ReduceOp.SUM, group=group)
    dist.all_reduce(confmat, op=dist.ReduceOp.SUM, group=group)
    loss_sum.copy_(lc[0])
    count.copy_(lc[1])
    return loss_sum, count, confmat


def shard_indices(n_items, rank, world, epoch_seed=0, shuffle=True, drop_last=False):
    """The partition Lightning's DistributedSampler gives the reference: a seeded
    permutation, padded to a multiple of ``world`` by wrapping, rank r takes r, r+W, r+2W, ..."""
    g = torch.Generator().manual_seed(epoch_seed)
    idx = torch.randperm(n_items, generator=g).tolist() if shuffle else list(range(n_items))
    if drop_last:
        idx = idx[: (n_items // world) * world]
    else:
        total = -(-n_items // world) * world
        idx = idx + idx[: total - len(idx)]
    return idx[rank::world]


def update_scales(lr, world, fold):
    """(lr, grad_scale) of one update from the gradient summed over ``world`` ranks."""
    # DDP's average is grad_scale = 1 / world on the gradient.  Folding it into lr instead -- p -= (lr / world) * sum of g, one
    # rounding fewer, what a trainer built with neither optimizer= nor clip_grad_norm= computes -- is only right for the rule without
    # weight decay and without momentum: decay would be scaled down with the step, a momentum buffer would hold (and save) sums
    # for averages, and Adam's step does not scale with its gradient at all.  The two differ in the last bit when world is no
    # power of two, so neither replaces the other.
    return (lr / world, 1.0) if fold else (lr, 1.0 / world)


class SegTrainer:
    """Owns the flat gradient buffer, the fused head outputs and the RCCL exchange for one rank."""

    def __init__(self, model, lr, class_weight=None, group=None, overlap=True, min_bucket_elems=1 << 18,
                 force_exchange=False, broadcast_buffers=True, class_names=None, metadata_encoder=None,
                 optimizer=None, clip_grad_norm=None, params=None, loss=None):
        """``optimizer``: a ``flair_amd.optim.SGD`` / ``AdamW`` specification; ``clip_grad_norm``: clip_grad_norm_'s max_norm over
        the U-Net's and the MetadataMLP's gradients together; ``params``: the parameter order of ``optimizer_state_dict()``
        (default ``list(model.parameters()) + list(metadata_encoder.parameters())``).  With neither of the first two the step is
        the reference's plain SGD (tasks_utils.py:95), ``optim.SGD()`` through the same kernel, with ``optimizer`` left None and
        DDP's average folded into the step size (``update_scales``).
        ``loss``: a ``flair_amd.losses.SegLoss`` -- train_step and validate_step compute that objective (flair_seg_loss_nhwc /
        flair_seg_loss) in place of the reference's weighted cross entropy, and ``loss_terms`` holds [loss, CE, Dice] of the last
        train_step; None: the reference's criterion through flair_ce_head_nhwc, every line as before."""
        self.model = model
        if loss is not None and not isinstance(loss, _losses.SegLoss):
            raise TypeError("loss must be a flair_amd.losses.SegLoss specification (or None: the reference's cross entropy)")
        self.loss_spec = loss
        # a MetadataMLP (BASELINE config 4): train_step / validate_step / predict add its encoding to the bottleneck inside their one
        # native call; train_step(..., mtd) also trains it
        self.metadata_encoder = metadata_encoder
        self._drows = None
        self._mlp_synced = False
        self.mlp_grads = None
        self.class_names = None if class_names is None else [str(n) for n in class_names]
        self.sync_buffers = bool(broadcast_buffers)   # torch DDP's broadcast_buffers (tasks.py:83-88 keeps the default, True)
        self._src0 = 0 if group is None else dist.get_global_rank(group, 0)
        self.lr = float(lr)
        self.group = group
        self.world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
        # rehearsal switch: run the event / side-stream / RCCL exchange even with one rank (1-GPU test boxes)
        self.exchange = self.world > 1 or (force_exchange and dist.is_available() and dist.is_initialized())
        self._no_collective = self.world == 1 and os.environ.get("FLAIR_REHEARSE_NO_COLLECTIVE") == "1"

        self.overlap = overlap
        p = model.flat_parameters()
        dev = p.device
        self.grads = torch.zeros_like(p)
        self.class_weight = None if class_weight is None else torch.as_tensor(class_weight, dtype=torch.float32, device=dev)
        self.confmat = torch.zeros(model.classes, model.classes, dtype=torch.int64, device=dev)
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.loss_terms = None
        if loss is not None:
            self.loss_terms = torch.zeros(3, dtype=torch.float32, device=dev)
            self.loss = self.loss_terms[0]   # the device scalar stays the loss
            self._loss_c = ops.seg_loss_spec(loss)
        self.buckets = bucket_ranges(model.stage_ranges(), min_bucket_elems)
        self._dl = None
        self._preds = None
        self._ce_ws = None
        # validation accumulators (validate_step / validation_epoch_end): MulticlassJaccardIndex's confusion matrix and
        # MeanMetric's (sum of values, sum of weights), every batch with weight 1
        self.val_confmat = torch.zeros(model.classes, model.classes, dtype=torch.int64, device=dev)
        self.val_loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
        self.val_count = torch.zeros((), dtype=torch.float64, device=dev)
        self._val_preds = None
        self._val_ws = None
        if self.exchange:
            # HIGH priority: its own hardware queues (HIP multiplexes streams over a few queues per priority level; a
            # normal-priority stream can land on the caller's queue and serialise the collectives behind the backward
            # kernels they are meant to overlap), and a bucket's all-reduce is dispatched as soon as its stage event fires
            self.comm_stream = torch.cuda.Stream(device=dev, priority=-1)
            self.events = [torch.cuda.Event() for _ in range(7)]
            for e in self.events:
                e.record()  # materialise the hipEvent_t handles
            # bucket -> the stage whose completion makes it ready (its lowest stage)
            sr = model.stage_ranges()
            self._bucket_stage = [min(s for s, (b, e) in enumerate(sr) if b >= bb and e <= be and e > b) for bb, be in self.buckets]
            dist.broadcast(p, src=self._src0, group=group)  # DDP's initial parameter broadcast
            dist.broadcast(model.flat_buffers(), src=self._src0, group=group)
        self._fold = optimizer is None and clip_grad_norm is None   # the plain trainer: see update_scales
        self._init_optimizer(_optim.SGD() if optimizer is None else optimizer, clip_grad_norm, params)

    # ------------------------------------------------------------------------------ the update (flair_amd.optim)
    def _init_optimizer(self, spec, clip_grad_norm, params):
        if not isinstance(spec, (_optim.SGD, _optim.AdamW)):
            raise TypeError("optimizer must be a flair_amd.optim.SGD or AdamW specification (torch.optim objects drive the "
                            "LightningModule surface, not the fused trainer)")
        if clip_grad_norm is not None and not float(clip_grad_norm) > 0:
            raise ValueError(f"clip_grad_norm must be positive, got {clip_grad_norm}")
        m = self.model
        dev = self.grads.device
        self._spec = spec
        self.clip_grad_norm = None if clip_grad_norm is None else float(clip_grad_norm)
        self._opt = _optim.FlatOptimizer(spec, m.flat_parameters(), list(m.parameters()))
        self._mlp_opt = None
        self.grad_norm = self._coef = None
        if self.clip_grad_norm is not None:
            # the norm leaves out the padding between stages of the flat buffer (every stage starts on 4 floats): maximal runs of
            # tensors, each starting on a 16-byte boundary
            spans = sorted((self._opt.offset(p), self._opt.offset(p) + p.numel()) for p in m.parameters())
            runs = []
            for b, e in spans:
                if runs and runs[-1][1] == b:
                    runs[-1][1] = e
                else:
                    runs.append([b, e])
            self._norm_runs = [(b, e) for b, e in runs]
            self._sq = torch.zeros(1, dtype=torch.float64, device=dev)
            self._sq_partials = torch.empty(ops.grad_sqnorm_partials(), dtype=torch.float64, device=dev)
            self._clip = torch.zeros(2, dtype=torch.float32, device=dev)
            self.grad_norm = self._clip[0]
            self._coef = self._clip[1:2]
        enc = self.metadata_encoder
        self.optimizer = None   # the plain trainer shows none: its rule has no state to save
        if not self._fold:
            plist = list(params) if params is not None else list(m.parameters()) + ([] if enc is None else list(enc.parameters()))
            self.optimizer = _optim.TrainerOptimizer(spec, self._flat_optimizers, plist, lambda: self.lr,
                                                     lambda v: setattr(self, "lr", v))
        if enc is not None and all(p.device == dev for p in enc.parameters()):
            self._bind_mlp()

    def _flat_optimizers(self):
        return [o for o in (self._opt, self._mlp_opt) if o is not None]

    def _bind_mlp(self):
        """Make the MetadataMLP's trainable tensors views of one flat buffer, in parameters() order, and bind the second flat
        optimizer over it; state already held survives a rebind after the module was moved."""
        ps = [p for p in self.metadata_encoder.parameters() if p.requires_grad]
        offs = [0]
        for p in ps:
            offs.append(offs[-1] + p.numel())
        old = self._mlp_opt
        same = old is not None and len(old.params) == len(ps) and all(a is b for a, b in zip(old.params, ps))
        if same and _flat.aliased(old.flat, zip(ps, offs)):
            return
        if any(p.numel() % 4 for p in ps):
            raise ValueError("the flat optimizer takes tensors of whole 16-byte chunks (numel % 4 == 0)")
        new = _optim.FlatOptimizer(self._spec, _flat.bind([(p, o, p.shape) for p, o in zip(ps, offs)], offs[-1], self.grads.device), ps)
        if old is not None and len(old.params) == len(ps):   # same tensors at new addresses: the state moves along
            for a, b in zip(new.state, old.state):
                a.copy_(b)
            new.steps = old.steps
        self._mlp_opt = new

    def optimizer_state_dict(self):
        """torch.optim's format (``state``: momentum_buffer, or step / exp_avg / exp_avg_sq, clones shaped like their parameter;
        ``param_groups`` with torch's keys) over the ``params`` order: loads into torch.optim.SGD / AdamW over the same parameters."""
        if self.optimizer is None:
            raise ValueError("SegTrainer was built without optimizer= / clip_grad_norm=: plain SGD has no state")
        return self.optimizer.state_dict()

    def load_optimizer_state_dict(self, sd):
        if self.optimizer is None:
            raise ValueError("SegTrainer was built without optimizer= / clip_grad_norm=: plain SGD has no state")
        if self.metadata_encoder is not None:
            if any(p.device != self.grads.device for p in self.metadata_encoder.parameters()):
                raise ValueError("move the metadata_encoder to the trainer's device before loading optimizer state")
            self._bind_mlp()
        self.optimizer.load_state_dict(sd)

    def _step(self, rows):
        """The update, behind the waited-for all-reduces: the MetadataMLP's backward from the row gradient the native backward left
        in ``_drows`` and the exchange of its gradients, one norm over both gradients (when clipping), then one kernel per flat buffer."""
        m = self.model
        if m._flat_p is not self._opt.flat:
            if self._spec.n_state:
                raise RuntimeError("the model's flat parameter buffer was rebuilt (moved or re-flattened) behind the optimizer: "
                                   "build a new SegTrainer and load optimizer_state_dict() into it")
            steps = self._opt.steps   # a rule without state follows the buffer
            self._opt = _optim.FlatOptimizer(self._spec, m._flat_p, list(m.parameters()))
            self._opt.steps = steps
        lr, gs = update_scales(self.lr, self.world, self._fold)
        mlp = None
        if rows is not None and self._mlp_opt.params:
            ps = self._mlp_opt.params
            for p in ps:
                p.grad = None
            rows.backward(self._drows)
            # one flat buffer (every tensor's size is a multiple of 4 floats: whole 16-byte chunks for the kernel)
            mlp = torch.cat([p.grad.reshape(-1) for p in ps])
            if self.exchange and not self._no_collective:
                # after the backward, outside the overlapped buckets: some 22 KB, nothing to overlap
                dist.all_reduce(mlp, op=dist.ReduceOp.SUM, group=self.group)
            self.mlp_grads = mlp   # like ``grads``: the (summed) gradient of the last step, in parameters() order
            for p in ps:
                p.grad = None
        if self.clip_grad_norm is not None:
            acc = False
            for b, e in self._norm_runs:
                ops.grad_sqnorm_(self.grads[b:e], self._sq, self._sq_partials, accumulate=acc)
                acc = True
            if mlp is not None:
                ops.grad_sqnorm_(mlp, self._sq, self._sq_partials, accumulate=True)
            ops.clip_coef_(self._sq, self.clip_grad_norm, self._clip[0:1], self._coef, grad_scale=gs)
        self._opt.step(self.grads, lr, grad_scale=gs, coef=self._coef)
        if mlp is not None:
            self._mlp_opt.step(mlp, lr, grad_scale=gs, coef=self._coef)

    def _buffers(self, B, H, W):
        m = self.model
        ld = L.lib().flair_unet_head_ld(m._h)
        dt = L.torch_dtype(m._dt)
        if self._dl is None or self._dl.shape != (B * H * W, ld):
            dev = self.grads.device
            self._dl = torch.empty(B * H * W, ld, dtype=dt, device=dev)
            self._preds = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
            wsb = L.lib().flair_ce_workspace_bytes(B, H, W)
            if self.loss_spec is not None:
                wsb = L.lib().flair_seg_loss_workspace_bytes(B, m.classes, H, W)
            self._ce_ws = torch.empty(wsb + 256, dtype=torch.uint8, device=dev)
        return ld

    def train_step(self, img, labels, mtd=None, mtd_masks="auto"):
        """img (B,Cin,H,W) fp32 HIP tensor; labels (B,H,W) uint8/int or fp32 one-hot (B,C,H,W).  Returns the
        device scalar loss (no host sync).

        ``mtd``: (B,45) metadata vectors (BASELINE config 4, model.py:57-62).  ``metadata_encoder`` encodes them in whatever mode it
        is in — the trainer never switches it — and the encoding is added to the bottleneck inside the one native training forward
        (rows_f32 + drows_f32 of flair_unet_fwd_opts_t); the native backward returns its gradient, which goes through the MetadataMLP's own backward
        kernel, and the MLP's trainable tensors, views of one flat buffer, take the U-Net's update rule in one launch of the same
        kernel (tasks_utils.py:95 hands the optimizer ``model.parameters()``, the MLP included); their ``.grad`` is None afterwards.
        ``mtd_masks``: the three dropout masks of MetadataMLP.forward — "auto" draws them from torch's generator when the encoder is
        in training mode (none in eval mode), a list is taken as it is, None means no dropout.  With a process group rank 0's MLP
        parameters are broadcast once, at the first such step, and each step sums the MLP's gradients over the ranks in one flat
        all-reduce behind the backward.  Without ``mtd`` the step leaves the encoder alone, whether one was given or not."""
        with torch.cuda.device(self.grads.device):   # every native call below launches on the current device's stream
            return self._train_step(img, labels, mtd, mtd_masks)

    def _meta_rows_train(self, img, mtd, masks):
        """x_enc of model.py:58 with its autograd graph (a leaf-to-rows graph of one _MlpFn node per 256 samples)."""
        enc = self.metadata_encoder
        if enc is None:
            raise ValueError("SegTrainer was built without a metadata_encoder: pass the MetadataMLP to take metadata")
        check_metadata_tile(img)
        dev = self.grads.device
        if self.exchange and not self._mlp_synced:
            # DDP's initial broadcast covers the whole module: rank 0's MLP, once
            ps = [p.data for p in enc.parameters()]
            flat = torch.cat([p.reshape(-1) for p in ps])
            dist.broadcast(flat, src=self._src0, group=self.group)
            for p, v in zip(ps, flat.split([p.numel() for p in ps])):
                p.copy_(v.view_as(p))
        self._mlp_synced = True
        self._bind_mlp()   # before the forward: it and the backward see one storage
        with torch.enable_grad():
            rows = enc(mtd.to(dev), masks=masks)
        B = img.shape[0]
        if self._drows is None or self._drows.shape != (B, 16):
            self._drows = torch.empty(B, 16, dtype=torch.float32, device=dev)
        return rows

    def _train_step(self, img, labels, mtd=None, mtd_masks="auto"):
        m = self.model
        B, _, H, W = img.shape
        ld = self._buffers(B, H, W)
        rows = None if mtd is None else self._meta_rows_train(img, mtd, mtd_masks)
        # logits stay in the workspace, NHWC of the compute dtype
        m._c_forward(img, training=True, want_logits=False, train_rows=None if rows is None else (rows.detach(), self._drows))
        kind = 3 if labels.dtype == torch.float32 else ops._LABEL_KIND[labels.dtype]
        l = L.lib()
        if self.loss_spec is None:
            L.check(l.flair_ce_head_nhwc(l.flair_unet_logits_nhwc(m._h), m._dt, ld, L.ptr(labels.contiguous()), kind,
                                         L.ptr(self.class_weight), B, m.classes, H, W, L.ptr(self.loss), L.ptr(self._dl),
                                         L.ptr(self._preds), None, L.ptr(self.confmat), L.ptr(self._ce_ws), L.stream()),
                    "ce_head_nhwc")
        else:
            L.check(l.flair_seg_loss_nhwc(l.flair_unet_logits_nhwc(m._h), m._dt, ld, L.ptr(labels.contiguous()), kind,
                                          L.ptr(self.class_weight), B, m.classes, H, W, ctypes.byref(self._loss_c), L.ptr(self.loss_terms),
                                          L.ptr(self._dl), L.ptr(self._preds), None, L.ptr(self.confmat), L.ptr(self._ce_ws),
                                          L.stream()), "seg_loss_nhwc")
        if self.exchange and self.overlap:
            m._c_backward(dlogits_nhwc=self._dl, grads=self.grads, stage_events=self.events)
            works = []
            with torch.cuda.stream(self.comm_stream):
                for i, ((b, e), st) in enumerate(zip(self.buckets, self._bucket_stage)):
                    self.comm_stream.wait_event(self.events[st])
                    if self._no_collective:   # diagnostic (FLAIR_REHEARSE_NO_COLLECTIVE=1): stage events and waits only
                        continue
                    if i == 0 and self.sync_buffers:
                        # the first stage event lies behind the whole forward: this step's running statistics are final
                        works.append(dist.broadcast(m.flat_buffers(), src=self._src0, group=self.group, async_op=True))
                    works.append(dist.all_reduce(self.grads[b:e], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            for w in works:
                w.wait()
        else:
            m._c_backward(dlogits_nhwc=self._dl, grads=self.grads)
            if self.exchange:
                allreduce_buckets(self.grads, self.buckets, self.group)
                if self.sync_buffers:
                    dist.broadcast(m.flat_buffers(), src=self._src0, group=self.group)
        self._step(rows)
        m._eval.note_native_write()   # parameters changed behind torch's version counter
        return self.loss

    def _meta_rows(self, img, mtd):
        """x_enc of model.py:58 for an eval-mode forward: the MetadataMLP without dropout (masks=None), as Lightning's
        ``model.eval()`` makes the reference's; None without metadata."""
        if mtd is None:
            return None
        if self.metadata_encoder is None:
            raise ValueError("SegTrainer was built without a metadata_encoder: pass the MetadataMLP to take metadata")
        check_metadata_tile(img)
        return self.metadata_encoder(mtd.to(self.grads.device), masks=None).detach()

    @torch.no_grad()
    def predict(self, img, mtd=None, tta=None):
        """predict_step of the reference (task_module.py:206-213): (B,H,W) uint8 argmax(softmax(logits)); with ``mtd`` ((B,45)
        metadata vectors) the logits of the metadata branch (model.py:57-62).  ``tta`` ("flips", "d4" or a list of D4 transform
        codes, ``flair_amd.tta``): the class of the largest mean probability over those transforms of ``img`` instead."""
        m = self.model
        B, _, H, W = img.shape
        codes = tta_codes(tta)
        with torch.cuda.device(self.grads.device):
            rows = self._meta_rows(img, mtd)
            if codes is not None:
                return m.predict_classes(img, bottleneck_rows=rows, tta=codes)
            return self._predict(m, img, B, H, W, rows)

    def _predict(self, m, img, B, H, W, rows=None):
        preds = torch.empty(B, H, W, dtype=torch.uint8, device=img.device)
        # the argmax comes out of the head convolution's epilogue (or, for shapes its persistent kernel does not take, from the
        # separate pass over the NHWC logits inside the same native call): the logits never reach HBM
        m._c_forward(img, training=False, want_logits=False, preds=preds, rows=rows)
        return preds

    @torch.no_grad()
    def validate_step(self, img, labels, mtd=None):
        """validation_step of the reference (task_module.py:104-109) on the eval handle and the eval workspace, with the
        running statistics whatever ``model.training`` says: one native call, the loss term, the argmax and the confusion
        matrix increment come out of the head convolution's epilogue (the ce_ fields of flair_unet_fwd_opts_t).  img / labels as for train_step.
        Returns this batch's device scalar loss (no host sync), adds it to the running mean and the batch's confusion matrix to
        ``val_confmat``; the predictions stay in ``_val_preds``.  No parameter, buffer or training activation is touched.
        ``mtd``: (B,45) metadata vectors, encoded by ``metadata_encoder`` without dropout and added to the bottleneck inside the
        same native call (rows_f32)."""
        with torch.cuda.device(self.grads.device):
            return self._validate_step(img, labels, self._meta_rows(img, mtd))

    def _validate_step(self, img, labels, rows=None):
        m = self.model
        B, _, H, W = img.shape
        dev = self.grads.device
        if self._val_preds is None or self._val_preds.shape != (B, H, W):
            self._val_preds = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
            self._val_ws = torch.empty(L.lib().flair_ce_workspace_bytes(B, H, W) + 256, dtype=torch.uint8, device=dev)
        kind = 3 if labels.dtype == torch.float32 else ops._LABEL_KIND[labels.dtype]
        labels = labels.contiguous()
        if self.loss_spec is not None:
            # the objective of train_step on the eval forward's fp32 NCHW logits (Unet.eval_logits: the route that hands the logits
            # out whether the eval forward ran eagerly or as a replayed graph)
            terms, _, preds, _ = ops.seg_loss(m.eval_logits(img, bottleneck_rows=rows), labels, self.loss_spec, self.class_weight,
                                              want_dlogits=False, want_preds="u8", confmat=self.val_confmat)
            self._val_preds = preds
            loss = terms[0].clone()
            self.val_loss_sum += loss
            self.val_count += 1
            return loss
        loss = torch.empty((), dtype=torch.float32, device=dev)   # (a tensor of its own: the caller may keep every batch's)
        m._c_forward(img, training=False, want_logits=False,
                     ce=(L.ptr(labels), kind, L.ptr(self.class_weight), L.ptr(loss), L.ptr(self._val_preds),
                         L.ptr(self.val_confmat), L.ptr(self._val_ws)), rows=rows)
        self.val_loss_sum += loss
        self.val_count += 1
        return loss

    @torch.no_grad()
    def validation_epoch_end(self):
        """on_validation_epoch_end of the reference (task_module.py:111-154): with a process group the accumulators are
        first summed over the ranks; ``val_loss`` = mean of the batch losses, ``val_miou`` = support-weighted Jaccard,
        ``val_iou`` = per-class Jaccard (flair_jaccard), ``val_iou_named`` = the classes of non-zero weight by name (by index
        without ``class_names``).  Resets the accumulators."""
        with torch.cuda.device(self.grads.device):
            if self.world > 1:
                reduce_validation_state(self.val_loss_sum, self.val_count, self.val_confmat, self.group)
            per, weighted, _ = ops.jaccard(self.val_confmat)
            val_loss = (self.val_loss_sum / self.val_count).to(torch.float32)
            C = self.model.classes
            names = self.class_names if self.class_names is not None else list(range(C))
            cw = [1.0] * C if self.class_weight is None else self.class_weight.tolist()
            named = {n: float(v) for n, w, v in zip(names, cw, per.tolist()) if w != 0}
            self.val_confmat.zero_()
            self.val_loss_sum.zero_()
            self.val_count.zero_()
            return {"val_loss": val_loss, "val_miou": weighted, "val_iou": per, "val_iou_named": named}
