"""Action-recognition fine-tuning and linear probing of the v1 video tower: the training step of
v1/downstream/run_class_finetuning.py / run_class_linear.py (engine_for_finetuning.py:14-137, optim_factory.py) over the HIP engine.

    model = VisionTransformer(num_classes=174, drop_path_rate=0.1, ...)            # downstream/video_encoder_v1.py
    groups = param_groups(model, weight_decay=0.05, layer_decay=0.75)              # optim_factory.get_parameter_groups
    opt = FusedTorchAdamW(groups, model.store, lr=1e-3, model=model)               # torch.optim.AdamW arithmetic, one launch
    step = FinetuneStep(model, opt, clip_grad=5.0, update_freq=1, smoothing=0.1)
    for samples, targets in loader:
        for g in opt.param_groups:                                                 # engine_for_finetuning.py:48-53
            g["lr"] = lr_schedule[it] * g["lr_scale"]
        out = step.step(samples, targets)                                          # loss, logits, grad_norm, class_acc

One step: EngineV1.finetune_forward (all patches, stochastic depth from a counter-based per-step table, `norm` at the CLS rows,
`head`), tvts_soft_ce (soft targets as a host-side Mixup produces them, or labels with smoothing), EngineV1.finetune_backward,
and on every update_freq-th call tvts_grad_sumsq (global norm + clip coefficient, left on the device), tvts_adamw_torch and a
fill-kernel zero of the gradients.  Nothing in the step synchronises with the host; the returned values are device tensors.
The optimizer, FusedTorchAdamW, lives in tvts_amd/optim.py beside FusedHFAdamW (one shared base) and is re-exported here.

OUT OF SCOPE (not built here): mixup / cutmix and the augmentation stack (the host data pipeline: pass their soft targets in),
``ModelEma``, the fp16 loss scaler (the engine is bf16 with fp32 accumulation: there is no loss scale), DeepSpeed, the multi-GPU
gradient exchange for this step (the backward keeps its Engine._ready calls so that one can hook in), and hipGraph capture of it.
"""
from __future__ import annotations

import torch

from .. import hip as K
from ..optim import FusedTorchAdamW  # noqa: F401  (re-exported)

MAX_GROUPS = FusedTorchAdamW.MAX_GROUPS


# ---------------------------------------------------------------------------------------------- parameter groups
def num_layer_for_vit(name: str, num_max_layer: int) -> int:
    """optim_factory.get_num_layer_for_vit (:26-37): cls_token / pos_embed / patch_embed.* are layer 0, blocks.i.* layer i + 1 and
    EVERYTHING else -- temporal_embed, norm.*, head.* -- the last layer id"""
    if name in ("cls_token", "mask_token", "pos_embed") or name.startswith("patch_embed"):
        return 0
    if name.startswith("rel_pos_bias"):
        return num_max_layer - 1
    if name.startswith("blocks"):
        return int(name.split(".")[1]) + 1
    return num_max_layer - 1


def layer_scales(depth: int, layer_decay: float):
    """run_class_finetuning.py:372-374: layer_decay ** (depth + 1 - i) for i = 0 .. depth + 1"""
    return [layer_decay ** (depth + 1 - i) for i in range(depth + 2)]


def param_groups(model, weight_decay, layer_decay=1.0, skip_list=None, trainable="all"):
    """optim_factory.get_parameter_groups (:51-90) with the LayerDecayValueAssigner of run_class_finetuning.py:369-378: a list of
    {"name", "weight_decay", "params", "param_names", "lr_scale"} in first-seen order, names ``layer_%d_decay`` /
    ``layer_%d_no_decay``.  No decay: 1-D tensors, ``*.bias`` and the skip list (default: model.no_weight_decay()).  As in the
    script, layer ids are assigned only with layer_decay < 1 (:369-372); without, the groups are ``decay`` / ``no_decay`` with
    lr_scale 1.  trainable "head": the parameters run_class_linear.py leaves trainable (:342-346)."""
    flags = model.set_trainable(trainable)
    skip = model.no_weight_decay() if skip_list is None else skip_list
    depth = model.arch["layers"]
    scales = layer_scales(depth, layer_decay) if layer_decay < 1.0 else None
    groups = {}
    for name, p in model.named_parameters():
        if not flags[name]:
            continue  # frozen weights
        no_decay = p.dim() == 1 or name.endswith(".bias") or name in skip
        gname = "no_decay" if no_decay else "decay"
        scale = 1.0
        if scales is not None:
            lid = num_layer_for_vit(name, len(scales))
            gname, scale = "layer_%d_%s" % (lid, gname), scales[lid]
        g = groups.get(gname)
        if g is None:
            g = groups[gname] = dict(name=gname, weight_decay=0.0 if no_decay else weight_decay, params=[], param_names=[],
                                     lr_scale=scale)
        g["params"].append(p)
        g["param_names"].append(name)
    return list(groups.values())


# ---------------------------------------------------------------------------------------------- the step
class FinetuneStep:
    """train_one_epoch's loop body (engine_for_finetuning.py:55-123) without DeepSpeed / loss scaler.  ``trainable="head"`` is
    linear probing: the backward stops behind the head; build the optimizer from ``param_groups(..., trainable="head")``."""

    def __init__(self, model, optimizer: FusedTorchAdamW, clip_grad=None, update_freq=1, smoothing=0.0, trainable="all"):
        if model.num_classes <= 0:
            raise ValueError("FinetuneStep needs a model with a head (num_classes > 0)")
        if update_freq < 1 or not (0.0 <= smoothing < 1.0):
            raise ValueError("update_freq >= 1 and 0 <= smoothing < 1")
        self.model, self.opt, self.trainable = model, optimizer, trainable
        self.clip_grad = float(clip_grad) if clip_grad else 0.0
        self.update_freq, self.smoothing = int(update_freq), float(smoothing)
        model.set_trainable(trainable)
        dev = model.store.device
        self.norm_coef = torch.zeros(2, dtype=torch.float32, device=dev)
        self.norm_coef[1] = 1.0
        optimizer.norm_coef = self.norm_coef
        self.partial = torch.zeros(optimizer.chunk_group.numel(), dtype=torch.float32, device=dev)
        self.loss_cell = torch.zeros(1, dtype=torch.float32, device=dev)
        self.hits = torch.zeros(1, dtype=torch.int32, device=dev)
        self.calls = 0

    def _targets(self, targets, B, C, dev):
        if targets.dim() == 1 and not targets.is_floating_point():
            if targets.numel() != B:
                raise ValueError(f"targets: {targets.numel()} labels for {B} clips")
            if int(targets.min()) < 0 or int(targets.max()) >= C:
                raise IndexError(f"labels must lie in [0, {C})")
            return dict(labels=targets.to(dev, torch.int32).contiguous(), smoothing=self.smoothing)
        if tuple(targets.shape) != (B, C):
            raise ValueError(f"targets: int64 labels [{B}] or soft targets [{B}, {C}], got {tuple(targets.shape)}")
        return dict(soft_targets=targets.to(dev, torch.float32).contiguous())  # (a Mixup has applied the smoothing already)

    @torch.no_grad()
    def step(self, samples, targets):
        """samples: fp32 [B, 3, T, H, W] or uint8 [B, T, H0, W0, 3]; targets: int64 labels [B] or soft [B, C].
        -> dict(loss, logits, grad_norm, class_acc): device tensors; loss is the unscaled loss of this call (:70), grad_norm the
        global norm before clipping on a call that updates, else None."""
        m, eng, st = self.model, self.model.engine, self.model.store
        a, dev = eng.arch, st.device
        if samples.dim() != 5:
            raise ValueError(f"samples: expected a 5-D clip batch, got {tuple(samples.shape)}")
        if samples.dtype == torch.uint8:
            if samples.shape[-1] != 3 or samples.shape[2] < a["image"] or samples.shape[3] < a["image"]:
                raise ValueError(f"uint8 samples must be [B, T, H, W, 3] with H, W >= {a['image']}")
            v, T, cm = samples.to(dev).contiguous(), samples.shape[1], False
        else:
            if tuple(samples.shape[1:2] + samples.shape[3:]) != (3, a["image"], a["image"]):
                raise ValueError(f"samples must be fp32 [B, 3, T, {a['image']}, {a['image']}]")
            v, T, cm = samples.to(dev, torch.float32).contiguous(), samples.shape[2], True
        if T == 0 or T % a["tubelet"] or T > a["num_frames"]:
            raise ValueError(f"clips of {T} frames: need a multiple of {a['tubelet']}, at most {a['num_frames']}")
        B, C = v.shape[0], m.num_classes
        tk = self._targets(targets, B, C, dev)
        m._fresh_shadows()
        logits = eng.finetune_forward(v, B, T // a["tubelet"], channel_major=cm)
        dlogits, ws = eng._f("ft.dlogits", (B, C)), eng._f("ft.ce_ws", (2 * B,))
        K.zero_(self.loss_cell)
        K.soft_ce(logits, self.loss_cell, ws, scale=1.0 / self.update_freq, dlogits=dlogits, hits=self.hits, **tk)
        eng.finetune_backward(dlogits, self.trainable)
        self.calls += 1
        grad_norm = None
        if self.calls % self.update_freq == 0:
            K.grad_sumsq(st.grad, self.opt.chunk_group, self.partial, self.norm_coef, max_norm=self.clip_grad,
                         grad_scale=self.opt.grad_scale)
            self.opt.step()
            K.zero_(st.grad)
            grad_norm = self.norm_coef[0].clone()
        return dict(loss=self.loss_cell[0] * float(self.update_freq), logits=logits.clone(), grad_norm=grad_norm,
                    class_acc=self.hits[0].to(torch.float32) / B)
