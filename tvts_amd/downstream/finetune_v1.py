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

Mixup / CutMix (run_class_finetuning.py:408-416, engine_for_finetuning.py:58-59; on in the default recipe):

    mixup_fn = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1,
                     num_classes=174)                                              # v1/downstream/mixup.py:97-112
    plan = mixup_fn.draw(B, img)                                                   # host: the reference's np.random calls, in order
    out = step.step(samples, labels, mix=plan)                                     # fp32 [B, 3, T, H, W] or uint8 [B, T, H0, W0, 3]

The plan is a per-sample table (partner, mode, box, lam, 1 - lam); the tubelet gather mixes the two clips element by element in
front of its bf16 rounding (tvts_patch_gather_tube_cm_mix / _u8_mix: uint8 clips are cropped and normalised first, then mixed, in
the reference's arithmetic order) and tvts_mix_targets builds the soft targets from the labels.  No mixed clip is materialised.

One step: EngineV1.finetune_forward (all patches, stochastic depth from a counter-based per-step table, `norm` at the CLS rows,
`head`), tvts_soft_ce (soft targets -- passed in, or built by tvts_mix_targets from a plan --, or labels with smoothing),
EngineV1.finetune_backward,
and on every update_freq-th call tvts_grad_sumsq (global norm + clip coefficient, left on the device), tvts_adamw_torch and a
fill-kernel zero of the gradients.  Nothing in the step synchronises with the host; the returned values are device tensors.
The optimizer, FusedTorchAdamW, lives in tvts_amd/optim.py beside FusedHFAdamW (one shared base) and is re-exported here.

Linear probing with the script's optimizer (v1/scripts/linear_ssv2.sh: --opt sgd --lr 0.1 --momentum 0.9 --weight_decay 1e-9;
run_class_linear.py:342-346 leaves the head trainable, optim_factory.py:121-126 maps `sgd` / `nesterov` to
torch.optim.SGD(momentum=args.momentum, nesterov=True) and `momentum` to the same without Nesterov):

    args = Namespace(opt="sgd", lr=0.1, momentum=0.9, weight_decay=1e-9, opt_eps=None, opt_betas=None)
    opt = create_optimizer(args, model, trainable="head")                          # -> FusedTorchSGD over param_groups(..., "head")
    step = FinetuneStep(model, opt, update_freq=1, trainable="head")
    out = step.step(samples, targets)

FusedTorchSGD (tvts_amd/optim.py) is torch.optim.SGD's single-tensor arithmetic bit for bit -- every add(x, alpha=a) of it is one
fused multiply-add -- as one launch over the flat store (tvts_sgd_torch; with a ModelEma, its ema argument): 22 B per trained
element with momentum against AdamW's 30.  Its state is torch's (``momentum_buffer``), so checkpoints travel both ways.

The per-sample augmentation behind RandAugment (ssv2.py:186-227: Normalize, random-resized crop, flip, random erasing; on in the
default recipe, with --num_sample 2 views per clip):

    aug_fn = Augment(224, hflip=0.0, reprob=0.25, remode="pixel", recount=1, num_sample=2)   # ssv2.py:196-222
    plan = aug_fn.draw(Bs, H0, W0)                                                 # host: the reference's random / np.random calls
    out = step.step(frames_u8, labels.repeat_interleave(2), mix=mixup_fn.draw(len(plan), img), aug=plan)   # uint8 [Bs, T, H0, W0, 3]

The plan is a per-sample table (source clip, crop, flip, erase box, noise key); tvts_patch_gather_tube_u8_aug forms every element
from its four bilinear taps of the uint8 source frame, erases, mixes and rounds once.  No augmented clip is materialised, and
the views of one clip read the same uploaded frames.  The erase noise is a counter-based normal, not torch's CPU stream.

RandAugment in front of all of it (ssv2.py:174-184, --aa rand-m7-n4-mstd0.5-inc1 in the default recipe; rand_augment.py):

    ra_fn = RandAugment("rand-m7-n4-mstd0.5-inc1", interpolation="bicubic", input_size=224)   # video_transforms.create_random_augment
    aug_fn = Augment(224, ..., num_sample=2, randaug=ra_fn)                        # per view: the RandAugment draws, then crop / flip / erase
    out = step.step(frames_u8, labels.repeat_interleave(2), mix=..., aug=aug_fn.draw(Bs, H0, W0))

The draw makes the reference's calls on ``np.random`` and ``random`` in its order and does the level arithmetic in Python doubles;
the plan carries, per view, the active ops as finished coefficients (RAPlan).  The step uploads the source clips ONCE into the head
of a work tensor [Bs + 2 * B, T, H0, W0, 3] and runs the layers over its two view regions (tvts_randaug_hist / tvts_randaug_apply,
one launch pair per layer, csrc/randaug.hip) with the bytes PIL gives -- every op, bilinear and bicubic -- then points the
plan's source column at the clip each view ended in, so the gather above reads the augmented views unchanged.

Several GPUs (run_class_finetuning.py / run_class_linear.py wrap the model in DistributedDataParallel, :403-406 of the latter;
train_one_epoch's non-DeepSpeed path, engine_for_finetuning.py:55-123): one process per GPU, torch.distributed initialised as the
script does, and the same two lines -- no wrap.

    step = FinetuneStep(model, opt, clip_grad=5.0, update_freq=1)                  # data_parallel=None: on with more than one rank
    out = step.step(samples, targets, mix=..., aug=...)                            # this rank's shard; step.bytes_sent afterwards

What replaces the wrap: at construction the ranks agree, by checksum, on the model size, `trainable`, update_freq, clip_grad, the
payload and the optimizer's chunk / group table (a mismatch raises on EVERY rank, none is left inside a collective), then rank
0's fp32 masters (store.flat) are broadcast and the bf16 shadows re-derived from them -- replicas start equal, as behind DDP's
wrap-time broadcast.  Only the call that updates (calls % update_freq == 0) exchanges gradients: the reference all-reduces on
every micro-step, and since the average of sums is the sum of averages, ONE exchange of the accumulated buffer is the same update
with 1 / update_freq of the traffic.  On that call the engine's grad_ready hook is armed with dist.GradSync.reduce_range in front of
finetune_backward and disarmed behind it, so the ranges travel (asynchronously, SUM) under the remaining backward: the head first,
the blocks depth - 1 .. 0, then the embedding parameters and the final norm.  Frozen ranges never travel (Engine._ready hands over
trainable runs only; with trainable="head" the whole exchange is the head's range) and a call that only accumulates issues no
collective.  Then: GradSync.finish(), tvts_grad_sumsq with grad_scale = 1 / W, tvts_adamw_torch with the same grad_scale, the zero
fill -- so grad_norm is the global norm of the AVERAGED gradient, what clip_grad_norm_ sees behind DDP (utils.py:366), and the clip
coefficient is the same number on every rank.  `loss` and `class_acc` stay per-rank device tensors: the reference logs per-rank
values too, and the script's MetricLogger does the epoch-end reduction on the host, unchanged.  payload="bf16" (or
TVTS_GRAD_PAYLOAD=bf16, as for pretraining) sends the gradients as bf16, half the bytes; fp32 is the default and keeps the
reference's fp32 all-reduce.  Both transports of dist.transport() carry it; the native one stays opt-in (TVTS_COMM=native).
FinetuneStep.replicas_checksum() is a device int64 over the parameter bits: compare it across ranks to assert that the replicas
are still equal.  With one rank (or data_parallel=False) nothing of this exists: no collective is created and the step is the
single-process step bit for bit.

Random draws across ranks.  Stochastic depth: every rank draws its own masks -- the engine's seed carries a per-rank offset
(EngineV1._rank_offset), whether the process group exists when the model is built or is created afterwards (FinetuneStep adopts
the rank at construction, EngineV1.adopt_rank).  Resume: ``model.engine.drop_seed_base()`` is the rank-independent part of the
seed -- rank 0 writes it into the checkpoint, EVERY rank reads it back with ``set_drop_seed_base(base)`` and continues its own
mask sequence (loading rank 0's seed verbatim would give all ranks rank 0's masks).  The host draws (Mixup.draw, Augment.draw,
RandAugment) use the global ``random`` / ``np.random``, which the script seeds with ``args.seed + rank``
(run_class_finetuning.py:230): they differ per rank as in the reference and need nothing here.

Averaged weights (--model_ema, run_class_finetuning.py:55-58,345-352; engine_for_finetuning.py:84-85,97-98):

    model_ema = ModelEma(model, decay=0.9999, device='', resume='')                # timm.utils.ModelEma's signature
    step = FinetuneStep(model, opt, ..., model_ema=model_ema)                      # every updating call also carries the average
    with model_ema.applied():                                                      # the model evaluates from the averaged weights
        stats = validation_one_epoch(loader, model)
    checkpoint["model_ema"] = model_ema.state_dict()                               # get_state_dict(model_ema), utils.py:419-440

Not a second model: ONE fp32 buffer with the flat store's layout.  The rule is timm's expression ``ema * decay + (1. - decay) * p`` on
fp32 tensors with a Python-float decay, bit for bit: ema' = fl(fl(ema * d32) + fl(o32 * p)), d32 = fp32(decay), o32 = fp32(1.0 -
decay) with the difference formed in double (hip.ema_pair).  With a FinetuneStep it rides in the optimizer's launch
(tvts_adamw_torch with ema, 38 instead of 30 B per trained element); ``update(model)`` is the same rule as a launch of its own
(tvts_ema_update) for a loop that calls it the way the reference does.  A chunk the optimizer does not step (group byte 255: the
whole tower under trainable="head", and padding) keeps every bit of its average, which is the parameter's value -- timm would let
it drift.  ``applied()`` exchanges the masters and the average in place (tvts_swap_f32_shadow) and re-derives the
shadows, on entry and again on exit: no second ParamStore, no second set of engine workspaces.

The epoch loop (run_class_finetuning.py main(), engine_for_finetuning.py:22-137, utils.py:399-503) and the overflow guard:

    step = FinetuneStep(model, opt, clip_grad=5.0, update_freq=1, model_ema=model_ema, skip_nonfinite=True)
    lr_values = cosine_scheduler(args.lr, args.min_lr, args.epochs, n_per_epoch, warmup_epochs=args.warmup_epochs)
    wd_values = cosine_scheduler(args.weight_decay, args.weight_decay_end, args.epochs, n_per_epoch)
    auto_load_model(args, model, opt, model_ema=model_ema, step=step)              # args.auto_resume: the newest checkpoint-<n>.pth
    for epoch in range(args.start_epoch, args.epochs):
        stats = train_one_epoch(step, loader, epoch, mixup_fn=mixup_fn, aug_fn=aug_fn, start_steps=epoch * n_per_epoch,
                                lr_schedule_values=lr_values, wd_schedule_values=wd_values,
                                num_training_steps_per_epoch=n_per_epoch, on_nonfinite="skip")
        save_model(args, epoch, model, opt, model_ema=model_ema, step=step)        # rank 0 writes, every rank calls

skip_nonfinite=True is GradScaler's "skip the update on inf / NaN", decided on the device: an updating call whose global gradient
norm (tvts_grad_sumsq's norm_coef[0]: over the trainable chunks, behind the all-reduce, 1 / W folded in) is not finite keeps every
bit of the masters, the moments (the momentum buffer), the shadows and the average, leaves the optimizer's device step counter where
it was and counts in ``step.skipped`` (device int64); the gradients are zeroed and grad_norm is returned as it is.  With a finite
norm the update is the unguarded update bit for bit.  The guarded launches (tvts_adamw_torch / tvts_sgd_torch with skipped) are the
chunk frames with one uniform load of the norm and a branch per block in front of every load of p / m / v; a one-lane kernel in
front of them advances the step counter or ``skipped``.  Every rank sees the same norm, so every rank decides alike and no
collective is added.  train_one_epoch reads the step's device scalars in one transfer every print_freq micro-steps, not on each
(the reference's loss.item()): on_nonfinite="stop" raises FloatingPointError at that readout, "skip" only counts.  Across ranks the
epoch's meters are merged through one dist.gather_rows table (counts and totals summed: SmoothedValue.synchronize_between_processes
+ global_avg).

OUT OF SCOPE (not built here): RandAugment's per-frame ``"random"`` interpolation and TranslateX / TranslateY (abs) (neither list of
rand_augment_transform holds them), --recount > 1,
``motion_shift`` (random_resized_crop_with_shift), the reference's torch noise stream,
``FastCollateMixup`` (the uint8-rounding variant: the reference scripts do not use it), ``ModelEma``'s ``device=`` (--model_ema_force_cpu)
and ``resume=`` arguments, the fp16 loss scaler (the engine is bf16 with fp32 accumulation: there is no loss scale), DeepSpeed,
sharded optimizer state, and hipGraph capture of the step.
The scripts' other half -- validation_one_epoch after every epoch, final_test over the test views and merge
(engine_for_finetuning.py:142-285), both across ranks too -- is tvts_amd/downstream/evaluate_v1.py.
"""
from __future__ import annotations

import contextlib
import math
import os
import random
import re
from typing import NamedTuple

import numpy as np
import torch

from .. import dist as D
from .. import hip as K
from ..engine import CH
from ..optim import FusedTorchAdamW, FusedTorchSGD  # noqa: F401  (re-exported)

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
    if not layer_decay < 1.0:
        return _factory_groups(model, weight_decay, skip_list, None, None, trainable)
    assigner = LayerDecayValueAssigner(layer_scales(model.arch["layers"], layer_decay))
    return _factory_groups(model, weight_decay, skip_list, assigner.get_layer_id, assigner.get_scale, trainable)


class LayerDecayValueAssigner:
    """optim_factory.LayerDecayValueAssigner (:40-48): get_layer_id / get_scale are what the scripts hand to create_optimizer as
    get_num_layer / get_layer_scale (run_class_finetuning.py:369-378)"""

    def __init__(self, values):
        self.values = values

    def get_scale(self, layer_id):
        return self.values[layer_id]

    def get_layer_id(self, var_name):
        return num_layer_for_vit(var_name, len(self.values))


_BUILT_OPTS = "adamw; sgd / nesterov (torch.optim.SGD with Nesterov momentum); momentum (torch.optim.SGD without)"


def create_optimizer(args, model, get_num_layer=None, get_layer_scale=None, filter_bias_and_bn=True, skip_list=None, trainable="all"):
    """optim_factory.create_optimizer (:93-178) for the optimizers the shipped scripts select: ``adamw`` -> FusedTorchAdamW, ``sgd`` /
    ``nesterov`` -> FusedTorchSGD(momentum=args.momentum, nesterov=True), ``momentum`` -> the same without Nesterov (:121-130); as
    there the name is lower-cased and only what follows its last ``_`` selects.  With args.weight_decay and filter_bias_and_bn
    the groups carry the decay (``param_groups``: get_parameter_groups with get_num_layer / get_layer_scale, a
    LayerDecayValueAssigner's bound methods or None) and the optimizer's own weight_decay is 0 (:96-103); else all trainable
    parameters form one group.  opt_eps is dropped for SGD (:122,125); opt_betas with an SGD name is refused (torch.optim.SGD would
    raise on the keyword).  Every other name -- and a ``lookahead_`` prefix -- raises NotImplementedError.  trainable: as
    ``param_groups`` ("head": the parameters run_class_linear.py leaves trainable)."""
    opt_lower = args.opt.lower()
    weight_decay = args.weight_decay
    flags = model.set_trainable(trainable)
    if weight_decay and filter_bias_and_bn:
        parameters = _factory_groups(model, weight_decay, skip_list, get_num_layer, get_layer_scale, trainable)
        weight_decay = 0.
    else:
        parameters = [p for n, p in model.named_parameters() if flags[n]]
    opt_args = dict(lr=args.lr, weight_decay=weight_decay)
    if getattr(args, "opt_eps", None) is not None:
        opt_args["eps"] = args.opt_eps
    if getattr(args, "opt_betas", None) is not None:
        opt_args["betas"] = args.opt_betas
    opt_split = opt_lower.split("_")
    opt_lower = opt_split[-1]
    if len(opt_split) > 1:
        raise NotImplementedError(f"create_optimizer(opt={args.opt!r}): prefixes (lookahead_) are not built; built: {_BUILT_OPTS}")
    if opt_lower in ("sgd", "nesterov", "momentum"):
        opt_args.pop("eps", None)
        if "betas" in opt_args:
            raise TypeError(f"create_optimizer(opt={args.opt!r}): opt_betas with an SGD optimizer (torch.optim.SGD has no betas)")
        return FusedTorchSGD(parameters, model.store, momentum=args.momentum, nesterov=opt_lower != "momentum", model=model, **opt_args)
    if opt_lower == "adamw":
        if "betas" in opt_args:
            opt_args["betas"] = tuple(opt_args["betas"])
        return FusedTorchAdamW(parameters, model.store, model=model, **opt_args)
    raise NotImplementedError(f"create_optimizer(opt={args.opt!r}) is not built; built: {_BUILT_OPTS}")


def _factory_groups(model, weight_decay, skip_list, get_num_layer, get_layer_scale, trainable):
    """get_parameter_groups (:51-90) as create_optimizer calls it, the one builder of the groups: without the two callables the
    groups are ``decay`` / ``no_decay`` with lr_scale 1; with them layer ids and scales come from the callables (a
    LayerDecayValueAssigner's give the groups of ``param_groups(..., layer_decay)``)"""
    flags = model.set_trainable(trainable)
    skip = model.no_weight_decay() if skip_list is None else skip_list
    groups = {}
    for name, p in model.named_parameters():
        if not flags[name]:
            continue  # frozen weights
        no_decay = p.dim() == 1 or name.endswith(".bias") or name in skip
        gname, lid = "no_decay" if no_decay else "decay", None
        if get_num_layer is not None:
            lid = get_num_layer(name)
            gname = "layer_%d_%s" % (lid, gname)
        g = groups.get(gname)
        if g is None:
            scale = get_layer_scale(lid) if get_layer_scale is not None else 1.
            g = groups[gname] = dict(name=gname, weight_decay=0.0 if no_decay else weight_decay, params=[], param_names=[], lr_scale=scale)
        g["params"].append(p)
        g["param_names"].append(name)
    return list(groups.values())


# ---------------------------------------------------------------------------------------------- Mixup / CutMix
class MixPlan(NamedTuple):
    """one step's draw, on the host: mix_i int32 [B, 6] = (partner, mode, yl, yh, xl, xh) with mode 0 none / 1 mixup / 2 cutmix /
    3 pair-mode cutmix, mix_f float32 [B, 2] = (lam, one_minus_lam), and the label smoothing of the soft targets.
    Mode 3: `_mix_pair` pastes `x[i][:, yl:yh, xl:xh]` (mixup.py:180-181), written for [C, H, W] pictures; on the [C, T, H, W] clips
    of this recipe the two slices land on (frame, row), and that is what the reference trains on in pair mode: the box (drawn
    for the picture, lam corrected for it) cuts the frames [yl, yh) and the rows [xl, xh), over the whole width."""
    mix_i: np.ndarray
    mix_f: np.ndarray
    smoothing: float


class Mixup:
    """v1/downstream/mixup.py:83-211 (timm's Mixup) split in two: ``draw`` makes the reference's random draws on the host and
    returns them as a MixPlan; the mixing itself runs inside the step's gather (FinetuneStep.step(..., mix=plan)).  Constructor
    keywords, defaults and ``mixup_enabled`` as the reference class (:97-112)."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch', correct_lam=True,
                 label_smoothing=0.1, num_classes=1000):
        if cutmix_minmax is not None:
            if len(cutmix_minmax) != 2:
                raise ValueError("cutmix_minmax: (min, max)")
            cutmix_alpha = 1.0  # (:102-105: min / max boxes do not use the alpha, the class forces it on)
        if mode not in ("batch", "pair", "elem"):
            raise ValueError("mode: 'batch', 'pair' or 'elem'")
        self.mixup_alpha, self.cutmix_alpha, self.cutmix_minmax = mixup_alpha, cutmix_alpha, cutmix_minmax
        self.mix_prob, self.switch_prob, self.label_smoothing, self.num_classes = prob, switch_prob, label_smoothing, num_classes
        self.mode, self.correct_lam, self.mixup_enabled = mode, correct_lam, True

    # the draws below call the GLOBAL np.random in the reference's order (a script seeded the same way draws the same plan), and
    # keep the reference's number types: float64 / Python scalars in batch mode, float32 array elements in pair / elem mode
    def _lam_mix(self, size):
        """-> (lam_mix, use_cutmix) of _params_per_batch (:138-148, size None) / _params_per_elem (:118-130)"""
        both = self.mixup_alpha > 0. and self.cutmix_alpha > 0.
        if not both and not self.mixup_alpha > 0. and not self.cutmix_alpha > 0.:
            raise ValueError("one of mixup_alpha > 0, cutmix_alpha > 0, cutmix_minmax must be set")
        if size is None:
            cut = bool(np.random.rand() < self.switch_prob) if both else not self.mixup_alpha > 0.
            alpha = self.cutmix_alpha if cut else self.mixup_alpha
            return np.random.beta(alpha, alpha), cut
        if both:  # both betas are drawn for every element, the cutmix one first
            cut = np.random.rand(size) < self.switch_prob
            lam_c = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=size)
            lam_m = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=size)
            return np.where(cut, lam_c, lam_m), cut
        alpha = self.mixup_alpha if self.mixup_alpha > 0. else self.cutmix_alpha
        return np.random.beta(alpha, alpha, size=size), np.full(size, not self.mixup_alpha > 0., dtype=bool)

    def _box(self, img, lam):
        """cutmix_bbox_and_lam (:70-80) on an img x img picture -> ((yl, yh, xl, xh), lam)"""
        if self.cutmix_minmax is not None:  # rand_bbox_minmax (:60-66)
            lo, hi = int(img * self.cutmix_minmax[0]), int(img * self.cutmix_minmax[1])
            cut_h = np.random.randint(lo, hi)
            cut_w = np.random.randint(lo, hi)
            yl = np.random.randint(0, img - cut_h)
            xl = np.random.randint(0, img - cut_w)
            yh, xh = yl + cut_h, xl + cut_w
        else:                               # rand_bbox (:36-45), margin 0; `ratio` keeps lam's type (float32 in pair / elem mode)
            ratio = np.sqrt(1 - lam)
            cut = int(img * ratio)
            cy = np.random.randint(0, img)
            cx = np.random.randint(0, img)
            yl, yh = np.clip(cy - cut // 2, 0, img), np.clip(cy + cut // 2, 0, img)
            xl, xh = np.clip(cx - cut // 2, 0, img), np.clip(cx + cut // 2, 0, img)
        if self.correct_lam or self.cutmix_minmax is not None:
            lam = 1. - ((yh - yl) * (xh - xl)) / float(img * img)
        return (int(yl), int(yh), int(xl), int(xh)), lam

    def draw(self, B, img):
        """the parameters of one step for B clips of img x img pixels -> MixPlan.  Odd B: ValueError (the reference asserts, :203)"""
        if B % 2:
            raise ValueError("Mixup needs an even batch size")
        mix_i = np.zeros((B, 6), dtype=np.int32)
        mix_i[:, 0] = B - 1 - np.arange(B)  # every mode mixes sample i with sample B - 1 - i (flip(0), :157,174,196)
        mix_f = np.empty((B, 2), dtype=np.float32)
        mix_f[:, 0], mix_f[:, 1] = 1.0, 0.0
        if self.mode == "batch":  # _mix_batch (:189-200): one draw for all; lam a double, 1 - lam taken in double
            lam, cut = 1., False
            if self.mixup_enabled and np.random.rand() < self.mix_prob:
                lam, cut = self._lam_mix(None)
                lam = float(lam)
            if lam != 1.:
                box = (0, 0, 0, 0)
                if cut:
                    box, lam = self._box(img, lam)
                mix_i[:, 1], mix_i[:, 2:] = 2 if cut else 1, box
                mix_f[:, 0], mix_f[:, 1] = np.float32(lam), np.float32(1. - lam)
            return MixPlan(mix_i, mix_f, float(self.label_smoothing))
        # _mix_elem (:152-167) / _mix_pair (:169-187): lam lives in a float32 array, 1 - lam is taken in float32
        n = B // 2 if self.mode == "pair" else B
        lam_batch, cut = np.ones(n, dtype=np.float32), np.zeros(n, dtype=bool)
        if self.mixup_enabled:
            lam_mix, cut = self._lam_mix(n)
            lam_batch = np.where(np.random.rand(n) < self.mix_prob, lam_mix.astype(np.float32), lam_batch)
        for i in range(n):
            lam = lam_batch[i]
            if lam == 1.:
                continue
            rows = (i, B - 1 - i) if self.mode == "pair" else (i,)
            if cut[i]:
                box, lam = self._box(img, lam)
                lam_batch[i] = lam
                for r in rows:
                    mix_i[r, 1], mix_i[r, 2:] = 3 if self.mode == "pair" else 2, box
            else:
                for r in rows:
                    mix_i[r, 1] = 1
            for r in rows:
                mix_f[r, 0], mix_f[r, 1] = lam_batch[i], np.float32(1) - lam_batch[i]
        return MixPlan(mix_i, mix_f, float(self.label_smoothing))


# ---------------------------------------------------------------------------------------------- RandAugment: the draw
# op codes of the plan's ra_i column 0, as tvts_randaug_apply reads them (include/tvts_hip.h)
(RA_NONE, RA_AUTOCONTRAST, RA_EQUALIZE, RA_INVERT, RA_SOLARIZE, RA_SOLARIZE_ADD, RA_POSTERIZE, RA_COLOR, RA_CONTRAST, RA_BRIGHTNESS,
 RA_SHARPNESS, RA_AFFINE) = range(12)
RA_STATS = (RA_AUTOCONTRAST, RA_EQUALIZE, RA_CONTRAST)  # the ops that read the frame's histograms (tvts_randaug_hist)
RA_MAX_LAYERS = 8
RA_BILINEAR, RA_BICUBIC = 2, 3  # PIL's Image.BILINEAR / Image.BICUBIC
_RA_MAX_LEVEL = 10.0
# rand_augment.py:385-420: the op of every slot as (reference function, level rule, level rule under `inc`)
_RA_OPS = (("auto_contrast", None, None), ("equalize", None, None), ("invert", None, None), ("rotate", "rotate", "rotate"),
           ("posterize", "posterize", "posterize_inc"), ("solarize", "solarize", "solarize_inc"),
           ("solarize_add", "solarize_add", "solarize_add"), ("color", "enhance", "enhance_inc"),
           ("contrast", "enhance", "enhance_inc"), ("brightness", "enhance", "enhance_inc"), ("sharpness", "enhance", "enhance_inc"),
           ("shear_x", "shear", "shear"), ("shear_y", "shear", "shear"), ("translate_x_rel", "translate_rel", "translate_rel"),
           ("translate_y_rel", "translate_rel", "translate_rel"))
# _RAND_CHOICE_WEIGHTS_0 (:425-441) in the order of _RAND_TRANSFORMS, the list _select_rand_weights indexes whatever list is in use
_RA_WEIGHTS_0 = (0.025, 0.005, 0, 0.3, 0, 0.005, 0.005, 0.025, 0.005, 0.005, 0.025, 0.2, 0.2, 0.1, 0.1)
_RA_BLEND = {"color": RA_COLOR, "contrast": RA_CONTRAST, "brightness": RA_BRIGHTNESS, "sharpness": RA_SHARPNESS}


def _negate(v):
    """_randomly_negate (:195-197)"""
    return -v if random.random() > 0.5 else v


def _ra_level(rule, level):
    """LEVEL_TO_ARG (:200-306) in the reference's Python doubles -> the one argument the op function receives"""
    if rule == "rotate":
        return _negate((level / _RA_MAX_LEVEL) * 30.0)
    if rule == "enhance":
        return (level / _RA_MAX_LEVEL) * 1.8 + 0.1
    if rule == "enhance_inc":
        return 1.0 + _negate((level / _RA_MAX_LEVEL) * 0.9)
    if rule == "shear":
        return _negate((level / _RA_MAX_LEVEL) * 0.3)
    if rule == "translate_rel":
        return _negate((level / _RA_MAX_LEVEL) * 0.45)
    if rule == "posterize":
        return int((level / _RA_MAX_LEVEL) * 4)
    if rule == "posterize_inc":
        return 4 - int((level / _RA_MAX_LEVEL) * 4)
    if rule == "solarize":
        return int((level / _RA_MAX_LEVEL) * 256)
    if rule == "solarize_inc":
        return 256 - int((level / _RA_MAX_LEVEL) * 256)
    if rule == "solarize_add":
        return int((level / _RA_MAX_LEVEL) * 110)
    raise ValueError(rule)


def ra_row(fn, arg, resample, H0, W0):
    """one op of the reference -- the NAME_TO_OP function `fn` (:64-192) called with `arg` and `resample` on H0 x W0 frames -- as a
    plan row: ((op, resample, iarg, 0), (a, b, c, d, e, f, factor, 0)).  The coefficients are what PIL hands its C code: the AFFINE
    data of Image.transform as they are, the matrix of Image.rotate (angle % 360, -radians, cos / sin rounded to 15 places, the
    centre (W0 / 2, H0 / 2) carried through), the enhancers' factor.  An op that PIL returns unchanged (posterize to 8 bits or
    more) is op 0."""
    ri, rd = [RA_NONE, 0, 0, 0], [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    if fn in ("auto_contrast", "equalize", "invert"):
        ri[0] = {"auto_contrast": RA_AUTOCONTRAST, "equalize": RA_EQUALIZE, "invert": RA_INVERT}[fn]
    elif fn in ("solarize", "solarize_add", "posterize"):
        if int(arg) != arg:
            raise ValueError(f"{fn}: an integer argument")
        if fn == "posterize" and arg >= 8:
            return tuple(ri), tuple(rd)
        if not (0 <= arg <= 256):
            raise ValueError(f"{fn}: argument outside [0, 256]")
        ri[0], ri[2] = {"solarize": RA_SOLARIZE, "solarize_add": RA_SOLARIZE_ADD, "posterize": RA_POSTERIZE}[fn], int(arg)
    elif fn in _RA_BLEND:
        ri[0], rd[6] = _RA_BLEND[fn], float(arg)
    elif fn in ("shear_x", "shear_y", "translate_x_rel", "translate_y_rel", "rotate"):
        if resample not in (RA_BILINEAR, RA_BICUBIC):
            raise ValueError("resample: 2 (bilinear) or 3 (bicubic)")
        ri[0], ri[1] = RA_AFFINE, resample
        if fn == "shear_x":
            rd[1] = float(arg)
        elif fn == "shear_y":
            rd[3] = float(arg)
        elif fn == "translate_x_rel":
            rd[2] = float(arg * W0)
        elif fn == "translate_y_rel":
            rd[5] = float(arg * H0)
        else:  # Image.rotate(degrees, resample, fillcolor): no expand, centre and translate left at their defaults
            angle = -math.radians(arg % 360.0)
            cx, cy = W0 / 2.0, H0 / 2.0
            a, b = round(math.cos(angle), 15), round(math.sin(angle), 15)
            d, e = round(-math.sin(angle), 15), round(math.cos(angle), 15)
            c = a * -cx + b * -cy + 0.0
            f = d * -cx + e * -cy + 0.0
            rd[:6] = a, b, c + cx, d, e, f + cy
    else:
        raise ValueError(f"RandAugment op {fn!r}")
    if not all(math.isfinite(v) for v in rd):
        raise ValueError(f"{fn}: a coefficient that is not finite")
    return tuple(ri), tuple(rd)


class RAPlan(NamedTuple):
    """one step's RandAugment draw, on the host.  The ACTIVE ops of every view, compacted to the front of its row:
    ra_i int32 [B, L, 4] = (op code, resample, integer argument, 0), op 0 = none; ra_d float64 [B, L, 8] = (affine a..f, blend
    factor, 0); num_sample views per source clip; ops: per view, every op the reference called, as (function name, argument or
    None, resample) -- the record the tests compare, not read by the step."""
    ra_i: np.ndarray
    ra_d: np.ndarray
    num_sample: int
    ops: list


class RandAugment:
    """rand_augment_transform / AugmentOp.__call__ / RandAugment.__call__ (rand_augment.py:337-531, built by create_random_augment,
    video_transforms.py:621-654, for ssv2.py:174-184) as draws only: ``draw_view`` makes the reference's calls on the global
    ``np.random`` and ``random`` in its order and returns the ops it would run; the ops themselves run on the device
    (tvts_randaug_hist / tvts_randaug_apply, FinetuneStep.step(..., aug=plan)).  config_str: --aa, e.g. "rand-m7-n4-mstd0.5-inc1".
    ``inc0`` selects the increasing list like ``inc1``: the reference tests bool("0") (:515).  ``w0`` weights the choice by
    _RAND_CHOICE_WEIGHTS_0 in the order of the non-increasing names and draws without replacement (:470-475).  interpolation:
    --train_interpolation, "bilinear" or "bicubic"; "random" (a resample drawn per frame and op, :50-55) is not built.  input_size
    only sets translate_const, which no op of the two lists reads."""

    def __init__(self, config_str, interpolation="bicubic", input_size=224):
        if interpolation == "random":
            raise ValueError("interpolation 'random' (a resample drawn per frame and op) is not built")
        if interpolation not in ("bilinear", "bicubic"):
            raise ValueError("interpolation: 'bilinear' or 'bicubic'")
        config = str(config_str).split("-")
        if not str(config_str).startswith("rand") or config[0] != "rand":
            raise ValueError("config_str: 'rand-...' (e.g. rand-m7-n4-mstd0.5-inc1)")
        self.resample = RA_BILINEAR if interpolation == "bilinear" else RA_BICUBIC
        self.magnitude, self.num_layers, self.magnitude_std, self.increasing, weight_idx = _RA_MAX_LEVEL, 2, 0, False, None
        std_set = False
        for c in config[1:]:
            cs = re.split(r"(\d.*)", c)
            if len(cs) < 2:
                continue
            key, val = cs[:2]
            if key == "mstd":
                if not std_set:  # (hparams.setdefault: the first one holds)
                    self.magnitude_std, std_set = float(val), True
            elif key == "inc":
                if bool(val):
                    self.increasing = True
            elif key == "m":
                self.magnitude = int(val)
            elif key == "n":
                self.num_layers = int(val)
            elif key == "w":
                weight_idx = int(val)
        if not (1 <= self.num_layers <= RA_MAX_LAYERS):
            raise ValueError(f"n: 1 to {RA_MAX_LAYERS} layers")
        if weight_idx not in (None, 0):
            raise ValueError("w: only weight set 0 exists")
        self.input_size = input_size
        self.weights = None
        if weight_idx is not None:  # _select_rand_weights (:444-450)
            probs = [w for w in _RA_WEIGHTS_0]
            self.weights = probs / np.sum(probs)

    def draw_view(self, H0, W0):
        """the draws of one RandAugment.__call__ -> (rows, ops): the plan rows of the active ops, in order, and the record"""
        if H0 < 3 or W0 < 3:
            raise ValueError("RandAugment needs frames of at least 3 x 3")
        picks = np.random.choice(len(_RA_OPS), self.num_layers, replace=self.weights is None, p=self.weights)
        rows, ops = [], []
        for k in picks:
            fn, rule, rule_inc = _RA_OPS[int(k)]
            if random.random() > 0.5:  # AugmentOp.__call__ (:365): prob 0.5 for every op
                continue
            magnitude = self.magnitude
            if self.magnitude_std and self.magnitude_std > 0:
                magnitude = random.gauss(magnitude, self.magnitude_std)
            magnitude = min(_RA_MAX_LEVEL, max(0, magnitude))
            rule = rule_inc if self.increasing else rule
            arg = None if rule is None else _ra_level(rule, magnitude)
            ops.append((fn, arg, self.resample))
            ri, rd = ra_row(fn, arg, self.resample, H0, W0)
            if ri[0] != RA_NONE:
                rows.append((ri, rd))
        return rows, ops

    def draw(self, B, H0, W0, num_sample=1):
        """B views of H0 x W0 frames, nothing drawn between them -> RAPlan"""
        return ra_plan([self.draw_view(H0, W0) for _ in range(B)], self.num_layers, num_sample)


def ra_plan(views, L, num_sample):
    """[(rows, ops)] per view -> RAPlan with L layers"""
    ra_i, ra_d = np.zeros((len(views), L, 4), dtype=np.int32), np.zeros((len(views), L, 8), dtype=np.float64)
    ra_d[:, :, 0] = ra_d[:, :, 4] = 1.0
    for b, (rows, _) in enumerate(views):
        for j, (ri, rd) in enumerate(rows):
            ra_i[b, j], ra_d[b, j] = ri, rd
    return RAPlan(ra_i, ra_d, int(num_sample), [ops for _, ops in views])


# ---------------------------------------------------------------------------------------------- crop, flip, random erasing
_M64 = (1 << 64) - 1
EMODE = {"const": 1, "rand": 2, "pixel": 3}


def splitmix64(x: int) -> int:
    """the first output of a splitmix64 generator seeded with x: the finaliser of the device's counter-based generator
    (attention.hip::drop_keep) applied to x + 0x9E3779B97F4A7C15"""
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


class AugPlan:
    """one step's per-sample augmentation draw, on the host: aug_i int32 [B, 16] = (src, top, left, h, w, flip, emode, etop, eleft,
    eh, ew, key_lo, key_hi, 0, 0, 0), the table of tvts_patch_gather_tube_u8_aug (include/tvts_hip.h).  len(plan) = B.
    ra: the RAPlan of the same B views (Augment(..., randaug=...)), or None: no RandAugment in front of the crop."""

    def __init__(self, aug_i, ra=None):
        self.aug_i, self.ra = aug_i, ra

    def __len__(self):
        return int(self.aug_i.shape[0])


class Augment:
    """What v1/downstream/ssv2.py:196-227 draws per sample behind RandAugment, split from what it computes: ``draw`` makes the
    reference's calls on the reference's generators (Python ``random`` and the global ``np.random``) in its order and with its
    number types, and returns them as an AugPlan; Normalize, the bilinear resize of the crop, the flip and the erase run inside
    the step's gather (FinetuneStep.step(frames_u8, targets, aug=plan)).  hflip: the flip probability, 0 = no flip and no draw
    (ssv2.py:208 passes random_horizontal_flip=False for SSv2; the other data sets flip with 0.5).  reprob / remode / recount:
    --reprob / --remode / --recount; reprob 0 builds no RandomErasing and draws nothing (ssv2.py:38-40).  num_sample: --num_sample,
    the views per decoded clip, collated as neighbours (utils.multiple_samples_collate): sample s * num_sample + k is view k of
    source clip s.  noise_seed: the erase noise is NOT torch's CPU stream (random_erasing.py:11-24) but a counter-based normal
    keyed per sample, key = splitmix64(noise_seed) + the number of samples drawn before it; the key never touches ``random`` /
    ``np.random``, so the reference's draw sequence is not shifted.  randaug: a RandAugment, or None -- every view then draws
    its RandAugment ops first (ssv2.py:174-184 runs in front of the crop), then the crop, flip and erase."""

    def __init__(self, input_size, scale=(0.08, 1.0), ratio=(0.75, 1.3333), hflip=0.0, reprob=0.25, remode="pixel", recount=1,
                 num_sample=1, noise_seed=0, randaug=None):
        if recount != 1:
            # (the script passes num_splits=args.recount, ssv2.py:220: recount > 1 would also leave the first T // recount frames clean)
            raise ValueError("recount != 1 is not built (one erase box per sample)")
        if remode not in EMODE:
            raise ValueError("remode: 'const', 'rand' or 'pixel'")
        if input_size < 1 or num_sample < 1:
            raise ValueError("input_size >= 1 and num_sample >= 1")
        self.input_size, self.scale, self.ratio, self.hflip = int(input_size), tuple(scale), tuple(ratio), float(hflip)
        self.reprob, self.remode, self.recount, self.num_sample = reprob, remode, recount, int(num_sample)
        # RandomErasing's defaults (random_erasing.py:46-64): min_area 0.02, max_area 1/3, min_aspect 0.3, max_aspect 1 / 0.3
        self.min_area, self.max_area = 0.02, 1 / 3
        self.log_aspect_ratio = (math.log(0.3), math.log(1 / 0.3))
        self.noise_key, self.drawn = splitmix64(int(noise_seed) & _M64), 0
        self.randaug = randaug

    def _crop(self, height, width):
        """_get_param_spatial_crop (video_transforms.py:499-538; log_scale=True, switch_hw=False) -> (i, j, h, w)"""
        scale, ratio = self.scale, self.ratio
        for _ in range(10):
            area = height * width
            target_area = random.uniform(*scale) * area
            log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
            aspect_ratio = math.exp(random.uniform(*log_ratio))
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            np.random.uniform()  # (:517 `np.random.uniform() < 0.5 and switch_hw`: drawn on every try, never used)
            if 0 < w <= width and 0 < h <= height:
                i = random.randint(0, height - h)
                j = random.randint(0, width - w)
                return i, j, h, w
        in_ratio = float(width) / float(height)  # the central fallback
        if in_ratio < min(ratio):
            w = width
            h = int(round(w / min(ratio)))
        elif in_ratio > max(ratio):
            h = height
            w = int(round(h * max(ratio)))
        else:
            w, h = width, height
        return (height - h) // 2, (width - w) // 2, h, w

    def _erase(self, img_h, img_w):
        """RandomErasing._erase_cube (random_erasing.py:109-149) with count 1 -> (top, left, h, w) or None"""
        if random.random() > self.reprob:
            return None
        area = img_h * img_w
        for _ in range(100):
            target_area = random.uniform(self.min_area, self.max_area) * area / 1
            aspect_ratio = math.exp(random.uniform(*self.log_aspect_ratio))
            h = int(round(math.sqrt(target_area * aspect_ratio)))
            w = int(round(math.sqrt(target_area / aspect_ratio)))
            if w < img_w and h < img_h:
                top = random.randint(0, img_h - h)
                left = random.randint(0, img_w - w)
                return top, left, h, w
        return None

    def draw(self, Bs, H0, W0):
        """the parameters of one step for Bs decoded clips of H0 x W0 pixels -> AugPlan for B = Bs * num_sample samples"""
        if Bs < 1 or H0 < 1 or W0 < 1:
            raise ValueError("Bs, H0, W0 >= 1")
        img = self.input_size
        aug_i = np.zeros((Bs * self.num_sample, 16), dtype=np.int32)
        views = []
        for b in range(Bs * self.num_sample):
            row = aug_i[b]
            if self.randaug is not None:
                views.append(self.randaug.draw_view(H0, W0))
            row[0] = b // self.num_sample
            row[1:5] = self._crop(H0, W0)
            if self.hflip > 0:
                row[5] = int(np.random.uniform() < self.hflip)  # horizontal_flip (video_transforms.py:176)
            box = self._erase(img, img) if self.reprob > 0 else None
            if box is not None and box[2] > 0 and box[3] > 0:
                row[6], row[7:11] = EMODE[self.remode], box
            key = (self.noise_key + self.drawn) & _M64
            self.drawn += 1
            row[11:13] = np.array([key & 0xFFFFFFFF, key >> 32], dtype=np.uint32).view(np.int32)
        return AugPlan(aug_i, None if self.randaug is None else ra_plan(views, self.randaug.num_layers, self.num_sample))


# ---------------------------------------------------------------------------------------------- averaged weights
class ModelEma:
    """timm.utils.ModelEma (run_class_finetuning.py:345-352) over the flat store: ``flat`` is ONE fp32 buffer with the layout of
    ``model.store.flat``, initialised as a bit copy of it.  Same constructor signature; a non-empty ``device`` (--model_ema_force_cpu)
    and a non-empty ``resume`` (the scripts pass '') are not built and are refused.  Handed to ``FinetuneStep(..., model_ema=...)``
    the average is updated inside the optimizer's launch on every updating call and the user does not call ``update``."""

    def __init__(self, model, decay=0.9999, device='', resume=''):
        if device:
            raise NotImplementedError(f"ModelEma(device={device!r}): an average on another device (--model_ema_force_cpu) is not built")
        if resume:
            raise NotImplementedError(f"ModelEma(resume={resume!r}): loading a checkpoint file is not built; use load_state_dict")
        decay = float(decay)
        if not (0.0 <= decay <= 1.0):
            raise ValueError(f"ModelEma(decay={decay!r}): expected a number in [0, 1]")
        self.model, self.decay = model, decay
        self.flat = model.store.flat.clone()
        self.chunk_group = None  # FinetuneStep hands over its optimizer's chunk table; alone, the table follows set_trainable()
        self._own_table = None
        self._active = False

    def _idle(self, what):
        if self._active:
            raise RuntimeError(f"ModelEma.{what} inside applied(): the masters and the average have changed places")

    def _chunks(self):
        """the chunk gate of update(): the optimizer's table when a FinetuneStep holds this average, else every chunk of a
        parameter the engine marks trainable (model.set_trainable) as group 0, all others 255"""
        if self.chunk_group is not None:
            return self.chunk_group
        st, flags = self.model.store, self.model.engine.requires_grad
        key = tuple(bool(flags[n]) for n in st.shapes)
        if self._own_table is None or self._own_table[0] != key:
            table = torch.full((st.total // CH,), 255, dtype=torch.uint8)
            for n, on in zip(st.shapes, key):
                if on:
                    o = st.off[n]
                    table[o // CH:(o + st._n(n) + CH - 1) // CH] = 0
            self._own_table = (key, table.to(st.device))
        return self._own_table[1]

    def reset(self):
        """the average becomes a bit copy of the masters again (FinetuneStep._join, behind the start-up broadcast)"""
        self._idle("reset")
        self.flat.copy_(self.model.store.flat)

    @torch.no_grad()
    def update(self, model=None):
        """ModelEma.update(model) as the reference's loop calls it (engine_for_finetuning.py:84-85,97-98): one launch of
        tvts_ema_update over the trainable chunks"""
        self._idle("update")
        if model is not None and model is not self.model:
            raise ValueError("ModelEma.update: the model this average was built from")
        K.ema_update(self.flat, self.model.store.flat, self._chunks(), self.decay)

    def _view(self, name):
        st = self.model.store
        o = st.off[name]
        return self.flat[o:o + st._n(name)].view(st.shapes[name])

    def state_dict(self):
        """clones of the averaged tensors under model.state_dict()'s keys and shapes: what get_state_dict(model_ema) puts into the
        checkpoint as `model_ema` (utils.py:419-440)"""
        self._idle("state_dict")
        return {k: self._view(self.model.store_name(k)).clone() for k in self.model.state_dict()}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        self._idle("load_state_dict")
        keys = list(self.model.state_dict())
        if set(state_dict) != set(keys):
            raise KeyError(f"ModelEma.load_state_dict: keys differ from the model's ({sorted(set(state_dict) ^ set(keys))[:4]} ...)")
        for k in keys:
            v, src = self._view(self.model.store_name(k)), state_dict[k]
            if tuple(src.shape) != tuple(v.shape):
                raise ValueError(f"ModelEma.load_state_dict: {k} has shape {tuple(src.shape)}, expected {tuple(v.shape)}")
            v.copy_(src)

    def checksum(self) -> torch.Tensor:
        """device int64 scalar: the sum of the average's bit patterns, as FinetuneStep.replicas_checksum() for the masters"""
        return self.flat.view(torch.int32).sum(dtype=torch.int64)

    def _exchange(self):
        st = self.model.store
        K.swap_f32_shadow(st.flat, self.flat, st.shadow)
        st.refresh_shadows(cast=False, transposed=True)
        self.model.mark_shadows_fresh()

    @contextlib.contextmanager
    def applied(self):
        """inside, the model evaluates from the averaged weights: model(x), forward_views, evaluate_v1.validation_one_epoch and
        final_test run unchanged.  Entry and exit are the same in-place exchange of masters and average (+ the shadows); behind
        it both hold their earlier bits, also when the body raised.  FinetuneStep.step, update, state_dict, load_state_dict and a
        nested applied() raise RuntimeError while it is active."""
        self._idle("applied")
        if getattr(self.model, "_ema_applied", None) is not None:
            raise RuntimeError("ModelEma.applied: another average is applied to this model")
        self._exchange()
        self._active, self.model._ema_applied = True, self
        try:
            yield self.model
        finally:
            self._active, self.model._ema_applied = False, None
            self._exchange()


# ---------------------------------------------------------------------------------------------- the step
class FinetuneStep:
    """train_one_epoch's loop body (engine_for_finetuning.py:55-123) without DeepSpeed / loss scaler.  ``trainable="head"`` is
    linear probing: the backward stops behind the head; build the optimizer from ``param_groups(..., trainable="head")`` or
    ``create_optimizer(args, model, trainable="head")``.  optimizer: FusedTorchAdamW or FusedTorchSGD (the script's probe).
    With more than one rank of torch.distributed it is the data-parallel step (module docstring, "Several GPUs")."""

    def __init__(self, model, optimizer: "FusedTorchAdamW | FusedTorchSGD", clip_grad=None, update_freq=1, smoothing=0.0, trainable="all",
                 data_parallel=None, payload=None, model_ema=None, skip_nonfinite=False):
        """skip_nonfinite: True -- every updating call decides ON THE DEVICE whether it updates: when the global gradient norm
        (after the all-reduce, over the trainable chunks) is not finite, the masters, the optimizer state, the shadows and the
        average keep every bit, the optimizer's device step counter stays and ``skipped`` counts one more (GradScaler's rule); the
        gradients are zeroed and grad_norm is returned as the non-finite value it is.  False: the step without a guard.
        model_ema: a ModelEma of this model -- every call that updates then also updates the average, inside the optimizer's
        launch (a call that only accumulates leaves it alone, as the reference's loop does); None: the step without an average.
        data_parallel: None -- on when torch.distributed is initialised with more than one rank; False -- the single-process
        step whatever the world size; True without a process group is refused.  payload: "fp32" (default) or "bf16", the number
        format the gradients travel in; None reads TVTS_GRAD_PAYLOAD, as the pretraining step does."""
        if payload not in (None, "fp32", "bf16"):
            raise ValueError(f"payload {payload!r}: expected 'fp32' or 'bf16' (None: TVTS_GRAD_PAYLOAD, default fp32)")
        if data_parallel and not (D.dist.is_available() and D.dist.is_initialized()):
            raise RuntimeError("data_parallel=True needs an initialised torch.distributed process group")
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
        self.skip_nonfinite = bool(skip_nonfinite)
        self.model_ema = model_ema
        if model_ema is not None:
            if model_ema.model is not model:
                raise ValueError("model_ema: a ModelEma built from this step's model")
            model_ema._idle("a FinetuneStep built")
            model_ema.chunk_group = optimizer.chunk_group
            optimizer.ema = (model_ema.flat, model_ema.decay)
        self.partial = torch.zeros(optimizer.chunk_group.numel(), dtype=torch.float32, device=dev)
        self.loss_cell = torch.zeros(1, dtype=torch.float32, device=dev)
        self.hits = torch.zeros(1, dtype=torch.int32, device=dev)
        self.calls = 0
        model.engine.adopt_rank()  # (a process group created after the model: the seed moves to this rank's mask sequence)
        self.world = D.world()[0]
        self.sync = None
        if self.world > 1 and (data_parallel is None or data_parallel):
            self._join(payload)

    def _join(self, payload):
        """what DistributedDataParallel does at wrap time: the ranks agree on what they are about to exchange, then take rank 0's
        parameters.  The agreement comes first -- ranks that disagree (another model, another `trainable`, another group table)
        all raise, none is left inside the broadcast."""
        st, opt = self.model.store, self.opt
        pay = payload or os.environ.get("TVTS_GRAD_PAYLOAD", "fp32")
        sig = repr((int(st.flat.numel()), self.trainable, self.update_freq, self.clip_grad, pay, len(opt.param_groups),
                    [float(g["weight_decay"]) for g in opt.param_groups], self.model.engine.recompute)).encode() + opt.chunk_group.cpu().numpy().tobytes()
        if self.model_ema is not None:  # (appended only with an average: without one the signature is the bytes it was)
            sig += repr(("model_ema", self.model_ema.decay)).encode()
        if not isinstance(opt, FusedTorchAdamW):  # (appended only for another optimizer: with AdamW the signature is the bytes it was)
            g0 = opt.param_groups[0]
            sig += repr((type(opt).__name__, float(g0.get("momentum", 0)), bool(g0.get("nesterov", False)))).encode()
        if self.skip_nonfinite:  # (appended only with the guard: without it the signature is the bytes it was)
            sig += repr(("skip_nonfinite", True)).encode()
        D.agree(sig, "FinetuneStep: the model size, `trainable`, update_freq, clip_grad, payload, the recomputation mode, the "
                     "ModelEma (present or not, its decay), the optimizer's kind (its momentum, nesterov), skip_nonfinite or the optimizer's chunk / group table")
        D.dist.broadcast(st.flat, src=0)
        st.refresh_shadows()
        self.model.mark_shadows_fresh()
        if self.model_ema is not None:  # an average made before the process group holds this rank's pre-broadcast weights
            self.model_ema.reset()
        self.sync = D.GradSync(st.grad, payload=pay)

    @property
    def bytes_sent(self) -> int:
        """the bytes this rank handed to the gradient exchange in the last call of step() (0: a call that only accumulated, or
        the single-process step)"""
        return 0 if self.sync is None else self.sync.bytes_sent

    @property
    def skipped(self) -> torch.Tensor:
        """device int64 [1]: the updating calls the overflow guard skipped so far (always 0 without skip_nonfinite)"""
        return self.opt.skipped

    def replicas_checksum(self) -> torch.Tensor:
        """device int64 scalar: the sum of the fp32 masters' bit patterns (store.flat read as int32, summed in int64).  Equal
        replicas give equal sums; compare it across ranks (or against a checkpoint) instead of the parameters.  No host sync."""
        return self.model.store.flat.view(torch.int32).sum(dtype=torch.int64)

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

    def _mixed_targets(self, targets, mix, B, C, img, dev):
        """the device table of a MixPlan and the soft targets tvts_mix_targets builds from the labels -> (table, soft_ce keywords)"""
        if targets.dim() != 1 or targets.is_floating_point() or targets.numel() != B:
            raise ValueError(f"with a mix plan the targets are integer labels [{B}]")
        if int(targets.min()) < 0 or int(targets.max()) >= C:
            raise IndexError(f"labels must lie in [0, {C})")
        if not (0.0 <= mix.smoothing < 1.0):
            raise ValueError("mix plan: 0 <= smoothing < 1")
        table = K.mix_table(mix.mix_i, mix.mix_f, B=B, img=img, device=dev)
        soft = self.model.engine._f("ft.mix_targets", (B, C))
        # (the plan's smoothing, not self.smoothing: with a mixup_fn the script's criterion is SoftTargetCrossEntropy, :421-423)
        K.mix_targets(targets.to(dev, torch.int32).contiguous(), table, soft, smoothing=mix.smoothing)
        return table, dict(soft_targets=soft)

    def _randaug(self, samples, aug, dev):
        """RandAugment in front of the gather: the source clips are uploaded ONCE into the head of a work tensor [Bs + 2 * B, T, H0,
        W0, 3], the layers run over its two view regions (hip.randaug_u8), and the plan's source column is rewritten to the clip
        every view ended in -- the gather then reads the augmented views like any source clips -> (work tensor, device aug table)"""
        Bs, T, H0, W0 = samples.shape[:4]
        B, ra = len(aug), aug.ra
        if ra.num_sample < 1 or B != Bs * ra.num_sample or ra.ra_i.shape[0] != B:
            raise ValueError(f"RandAugment plan: {ra.ra_i.shape[0]} views of {ra.num_sample} per clip for {Bs} clips, {B} samples")
        src = np.asarray(aug.aug_i)[:, 0]
        if (src != np.arange(B) // ra.num_sample).any():
            raise ValueError("with RandAugment, sample b is a view of source clip b // num_sample")
        table = K.RandaugTable(ra.ra_i, ra.ra_d, Bs=Bs, num_sample=ra.num_sample, device=dev)
        shape = (Bs + 2 * B, T, H0, W0, 3)
        if getattr(self, "_ra_work", None) is None or tuple(self._ra_work.shape) != shape:
            self._ra_work = torch.empty(shape, dtype=torch.uint8, device=dev)
            self._ra_hist = torch.empty((B, T, 4, 256), dtype=torch.int32, device=dev)
        work = self._ra_work
        work[:Bs].copy_(samples)
        rows = K.randaug_u8(work, table, self._ra_hist)
        aug_i = np.array(aug.aug_i, dtype=np.int64)
        aug_i[:, 0] = rows
        return work, K.aug_table(aug_i, Bs=Bs + 2 * B, H0=H0, W0=W0, img=self.model.engine.arch["image"], device=dev)

    @torch.no_grad()
    def step(self, samples, targets, mix=None, aug=None):
        """samples: fp32 [B, 3, T, H, W] or uint8 [B, T, H0, W0, 3]; targets: int64 labels [B] or soft [B, C].  mix: a MixPlan
        (Mixup.draw) -- targets are then integer labels, the clips are mixed inside the gather and the soft targets built on the
        device with the plan's label smoothing; None: no mixing.  aug: an AugPlan (Augment.draw) -- samples are then the uint8
        SOURCE frames [Bs, T, H0, W0, 3] (any H0, W0 >= 1), the step has B = len(aug) samples, each cropped, resized, flipped and
        erased inside the gather from the source clip its row names; targets has B entries (the caller repeats the labels as the
        collate does) and a MixPlan is drawn for B; None: uint8 clips take the centre crop, as before.  A plan that carries a
        RandAugment draw (Augment(..., randaug=...)) runs its ops on the device first, on the uploaded source frames (H0, W0 >= 3).
        -> dict(loss, logits, grad_norm, class_acc): device tensors; loss is the unscaled loss of this call (:70), grad_norm the
        global norm before clipping on a call that updates, else None.  Across ranks loss / logits / class_acc are this rank's,
        grad_norm is the norm of the gradient averaged over the ranks (the same value on every rank)."""
        m, eng, st = self.model, self.model.engine, self.model.store
        a, dev = eng.arch, st.device
        if getattr(m, "_ema_applied", None) is not None:
            raise RuntimeError("FinetuneStep.step inside ModelEma.applied(): the masters hold the averaged weights")
        if samples.dim() != 5:
            raise ValueError(f"samples: expected a 5-D clip batch, got {tuple(samples.shape)}")
        if aug is not None:
            if samples.dtype != torch.uint8 or samples.shape[-1] != 3 or min(samples.shape[:4]) < 1:
                raise ValueError("with an augmentation plan the samples are uint8 source frames [Bs, T, H0, W0, 3]")
            # (a RandAugment plan uploads the clips into its work tensor instead: _randaug below)
            v, T, cm = samples if aug.ra is not None else samples.to(dev).contiguous(), samples.shape[1], False
        elif samples.dtype == torch.uint8:
            if samples.shape[-1] != 3 or samples.shape[2] < a["image"] or samples.shape[3] < a["image"]:
                raise ValueError(f"uint8 samples must be [B, T, H, W, 3] with H, W >= {a['image']}")
            v, T, cm = samples.to(dev).contiguous(), samples.shape[1], False
        else:
            if tuple(samples.shape[1:2] + samples.shape[3:]) != (3, a["image"], a["image"]):
                raise ValueError(f"samples must be fp32 [B, 3, T, {a['image']}, {a['image']}]")
            v, T, cm = samples.to(dev, torch.float32).contiguous(), samples.shape[2], True
        if T == 0 or T % a["tubelet"] or T > a["num_frames"]:
            raise ValueError(f"clips of {T} frames: need a multiple of {a['tubelet']}, at most {a['num_frames']}")
        B, C = v.shape[0] if aug is None else len(aug), m.num_classes
        if aug is not None and aug.ra is not None:
            v, atab = self._randaug(samples, aug, dev)
        else:
            atab = None if aug is None else K.aug_table(aug.aug_i, Bs=v.shape[0], H0=v.shape[2], W0=v.shape[3], img=a["image"], device=dev)
        if mix is None:
            table, tk = None, self._targets(targets, B, C, dev)
        else:
            table, tk = self._mixed_targets(targets, mix, B, C, a["image"], dev)
        m._fresh_shadows()
        logits = eng.finetune_forward(v, B, T // a["tubelet"], channel_major=cm, mix=table, aug=atab)
        dlogits, ws = eng._f("ft.dlogits", (B, C)), eng._f("ft.ce_ws", (2 * B,))
        K.zero_(self.loss_cell)
        K.soft_ce(logits, self.loss_cell, ws, scale=1.0 / self.update_freq, dlogits=dlogits, hits=self.hits, **tk)
        updating = (self.calls + 1) % self.update_freq == 0
        sync, hook = self.sync, eng.grad_ready
        if sync is not None:
            sync.bytes_sent = 0
            if updating:  # the accumulated gradient travels once, range by range under the rest of this backward
                eng.grad_ready = sync.reduce_range
        try:
            eng.finetune_backward(dlogits, self.trainable)
        finally:
            eng.grad_ready = hook
        self.calls += 1
        grad_norm = None
        if updating:
            # behind the exchange the buffer holds the SUM over the ranks; 1 / W rides in the norm and in the update, so grad_norm
            # is the norm of the averaged gradient and the clip coefficient is the same number on every rank
            scale = self.opt.grad_scale if sync is None else self.opt.grad_scale * sync.finish()
            K.grad_sumsq(st.grad, self.opt.chunk_group, self.partial, self.norm_coef, max_norm=self.clip_grad, grad_scale=scale)
            kept, self.opt.grad_scale = self.opt.grad_scale, scale
            try:
                if self.skip_nonfinite:
                    self.opt.step(guard=True)
                else:
                    self.opt.step()
            finally:
                self.opt.grad_scale = kept
            K.zero_(st.grad)
            grad_norm = self.norm_coef[0].clone()
        return dict(loss=self.loss_cell[0] * float(self.update_freq), logits=logits.clone(), grad_norm=grad_norm,
                    class_acc=self.hits[0].to(torch.float32) / B)


# ---------------------------------------------------------------------------------------------- the epoch loop
METERS = ("loss", "class_acc", "lr", "min_lr", "weight_decay", "grad_norm", "skipped")  # the row order of the rank-merged table


def cosine_scheduler(base_value, final_value, epochs, niter_per_ep, warmup_epochs=0, start_warmup_value=0, warmup_steps=-1):
    """utils.cosine_scheduler (utils.py:399-416) in its float64 arithmetic -> ndarray [epochs * niter_per_ep]: a linear warm-up
    (np.linspace) over warmup_epochs * niter_per_ep iterations, or over warmup_steps when that is positive, then half a cosine
    from base_value to final_value.  Its quirk is kept: the warm-up values are only built with warmup_epochs > 0, so warmup_steps
    > 0 with warmup_epochs == 0 shortens the cosine part without adding a warm-up and fails the length assertion."""
    warmup_schedule = np.array([])
    warmup_iters = warmup_epochs * niter_per_ep
    if warmup_steps > 0:
        warmup_iters = warmup_steps
    if warmup_epochs > 0:
        warmup_schedule = np.linspace(start_warmup_value, base_value, warmup_iters)
    iters = np.arange(epochs * niter_per_ep - warmup_iters)
    schedule = np.array([final_value + 0.5 * (base_value - final_value) * (1 + math.cos(math.pi * i / (len(iters)))) for i in iters])
    schedule = np.concatenate((warmup_schedule, schedule))
    assert len(schedule) == epochs * niter_per_ep
    return schedule


def merge_train_meters(rows):
    """per-rank tables [len(METERS), 2] of (count, total) -> {meter: global_avg}: counts and totals summed over the ranks, then
    total / count, what SmoothedValue.synchronize_between_processes followed by global_avg does (utils.py:49-60,72-74).  A meter
    nobody updated (class_acc under Mixup, weight_decay without a decayed group) is absent, as in the reference's dict."""
    t = torch.as_tensor(rows, dtype=torch.float64).reshape(-1, len(METERS), 2).sum(0)
    return {k: float(t[i, 1]) / int(t[i, 0]) for i, k in enumerate(METERS) if int(t[i, 0]) > 0}


def train_one_epoch(step, data_loader, epoch, criterion=None, device=None, loss_scaler=None, mixup_fn=None, log_writer=None,
                    start_steps=0, lr_schedule_values=None, wd_schedule_values=None, num_training_steps_per_epoch=None,
                    update_freq=None, aug_fn=None, print_freq=10, on_nonfinite="stop"):
    """engine_for_finetuning.train_one_epoch (:22-137) over a FinetuneStep, which already holds the model, the optimizer, max_norm
    (clip_grad) and the ModelEma.  data_loader yields (samples, targets, ...); only the first two are read.  ``criterion``,
    ``device`` and ``loss_scaler`` are accepted for the reference's call shape and IGNORED: the loss is the step's soft-target /
    smoothed cross-entropy, the device is the model's, and there is no loss scale.  mixup_fn: a Mixup -- its draw is made per
    micro-step and handed to the step as ``mix``; aug_fn: an Augment -- samples are then uint8 source frames and the targets are
    repeated per view.  update_freq: None or the step's own value (another one is refused).

    Kept from the reference: micro-steps beyond num_training_steps_per_epoch * update_freq are drawn from the loader and dropped;
    ``it = start_steps + step``; the schedule assignment with the precedence of :47 -- with an lr schedule it runs on EVERY micro-
    step (same ``it``), with a weight-decay schedule alone only on the first micro-step of an update; lr is scaled by the group's
    lr_scale and only groups whose weight_decay is above 0 take the scheduled decay.  Returned: {meter: global_avg} under the
    reference's names loss, class_acc (absent with a mixup_fn), lr, min_lr, weight_decay, grad_norm; instead of loss_scale the
    dict carries ``skipped``, the guard's counter at the end of the epoch (cumulative, a state value as loss_scale was).

    Changed: the host does not read the device on every micro-step.  The step's device scalars are kept and read in ONE transfer
    whenever data_iter_step % print_freq == 0 (the reference's log_every rhythm) and once behind the last micro-step.  At that
    readout on_nonfinite="stop" raises FloatingPointError naming the first iteration whose loss or gradient norm was not finite,
    where the reference's sys.exit(1) would have fired; "skip" only counts, and leaves non-finite values out of the loss /
    grad_norm meters.  With FinetuneStep(skip_nonfinite=True) the weights are intact either way; without it "skip" is refused in
    front of the first micro-step (it would train on NaN).  Across ranks the meters are merged at the end of the epoch through
    one dist.gather_rows table (merge_train_meters)."""
    if on_nonfinite not in ("stop", "skip"):
        raise ValueError(f"on_nonfinite {on_nonfinite!r}: expected 'stop' or 'skip'")
    if on_nonfinite == "skip" and not getattr(step, "skip_nonfinite", False):
        raise ValueError("on_nonfinite='skip' needs FinetuneStep(skip_nonfinite=True): without the guard a non-finite gradient "
                         "is written into every weight and the loop would train on NaN")
    if update_freq is None:
        update_freq = step.update_freq
    if int(update_freq) != step.update_freq:
        raise ValueError(f"update_freq {update_freq}: the step was built with {step.update_freq}")
    if print_freq < 1:
        raise ValueError("print_freq >= 1")
    if num_training_steps_per_epoch is None:
        num_training_steps_per_epoch = len(data_loader) // update_freq
    opt = step.opt
    count, total = [0] * len(METERS), [0.0] * len(METERS)

    def meter(name, value):
        if value is not None:
            i = METERS.index(name)
            count[i] += 1
            total[i] += value

    pending = []  # (it, loss, class_acc or None, grad_norm or None, max lr, min lr, weight decay or None) of micro-steps not read yet

    def readout():
        """ONE device -> host transfer for everything pending (+ the skip counter); meters, log_writer, the non-finite rule"""
        if not pending:
            return 0
        cells = [step.skipped.reshape(-1)[0].to(torch.float64)]
        for _, loss, acc, gn, *_ in pending:
            cells += [c.to(torch.float64) for c in (loss, acc, gn) if c is not None]
        host = iter(torch.stack(cells).cpu().tolist())
        skipped = int(next(host))
        for it, loss, acc, gn, max_lr, min_lr, wd in pending:
            loss = next(host)
            acc = None if acc is None else next(host)
            gn = None if gn is None else next(host)
            bad = not math.isfinite(loss) or (gn is not None and not math.isfinite(gn))
            if bad and on_nonfinite == "stop":
                pending.clear()
                what = f"Loss is {loss}" if not math.isfinite(loss) else f"Gradient norm is {gn}"
                raise FloatingPointError(f"{what} at iteration {it} (epoch {epoch}), stopping training")
            meter("loss", loss if math.isfinite(loss) else None)
            meter("class_acc", acc)
            meter("lr", max_lr)
            meter("min_lr", min_lr)
            meter("weight_decay", wd)
            meter("grad_norm", gn if gn is None or math.isfinite(gn) else None)
            if log_writer is not None:
                log_writer.update(loss=loss, head="loss")
                log_writer.update(class_acc=acc, head="loss")
                log_writer.update(skipped=skipped, head="opt")
                log_writer.update(lr=max_lr, head="opt")
                log_writer.update(min_lr=min_lr, head="opt")
                log_writer.update(weight_decay=wd, head="opt")
                log_writer.update(grad_norm=gn, head="opt")
                log_writer.set_step()
        pending.clear()
        return skipped

    opt.zero_grad()
    skipped = 0
    for data_iter_step, batch in enumerate(data_loader):
        it_step = data_iter_step // update_freq
        if it_step >= num_training_steps_per_epoch:
            continue
        it = start_steps + it_step  # global training iteration
        if lr_schedule_values is not None or wd_schedule_values is not None and data_iter_step % update_freq == 0:
            for param_group in opt.param_groups:
                if lr_schedule_values is not None:
                    param_group["lr"] = lr_schedule_values[it] * param_group["lr_scale"]
                if wd_schedule_values is not None and param_group["weight_decay"] > 0:
                    param_group["weight_decay"] = wd_schedule_values[it]
        samples, targets = batch[0], batch[1]
        plan = None
        if aug_fn is not None:
            plan = aug_fn.draw(samples.shape[0], samples.shape[2], samples.shape[3])
            targets = targets.repeat_interleave(aug_fn.num_sample)
        mix = None
        if mixup_fn is not None:
            mix = mixup_fn.draw(samples.shape[0] if plan is None else len(plan), step.model.engine.arch["image"])
        out = step.step(samples, targets, mix=mix, aug=plan)
        min_lr, max_lr, wd = 10., 0., None
        for group in opt.param_groups:
            min_lr, max_lr = min(min_lr, group["lr"]), max(max_lr, group["lr"])
            if group["weight_decay"] > 0:
                wd = group["weight_decay"]
        pending.append((it, out["loss"], None if mixup_fn is not None else out["class_acc"], out["grad_norm"], float(max_lr),
                        float(min_lr), None if wd is None else float(wd)))
        if data_iter_step % print_freq == 0:
            skipped = readout()
    if pending:
        skipped = readout()
    else:
        skipped = int(step.skipped.reshape(-1)[0].item())
    meter("skipped", skipped)
    table = torch.tensor([[float(c), float(t)] for c, t in zip(count, total)], dtype=torch.float64)
    return merge_train_meters(D.gather_rows(table))


def save_model(args, epoch, model, optimizer, model_ema=None, step=None):
    """utils.save_model (:419-440), the branch without DeepSpeed: ``args.output_dir/checkpoint-<epoch>.pth`` written by rank 0 with
    the keys model, optimizer, epoch, args and -- with an average -- model_ema (ModelEma.state_dict(): get_state_dict(model_ema)).
    No ``scaler`` key: there is no loss scale.  For an exact continuation of THIS engine the file also carries drop_seed_base (the
    rank-independent part of the stochastic-depth seed, every rank reads it back) and, with a FinetuneStep, its ``calls`` and
    ``skipped``.  optimizer.state_dict() reads the device step counter: behind skipped updates it reports the updates that
    counted, and loads into torch.optim.AdamW / SGD.  Every rank calls it (the state dicts are formed on every rank alike)."""
    to_save = {"model": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "optimizer": optimizer.state_dict(),
               "epoch": epoch, "args": args, "drop_seed_base": int(model.engine.drop_seed_base())}
    if model_ema is not None:
        to_save["model_ema"] = {k: v.cpu() for k, v in model_ema.state_dict().items()}
    if step is not None:
        to_save["calls"], to_save["skipped"] = int(step.calls), int(step.skipped.reshape(-1)[0].item())
    if D.world()[1] == 0:
        os.makedirs(args.output_dir, exist_ok=True)
        torch.save(to_save, os.path.join(args.output_dir, "checkpoint-%s.pth" % str(epoch)))


def auto_load_model(args, model, optimizer, model_ema=None, step=None):
    """utils.auto_load_model (:444-475), the branch without DeepSpeed, on EVERY rank: args.auto_resume with an empty args.resume
    picks ``checkpoint-<n>.pth`` with the largest all-digit n in args.output_dir (checkpoint-best.pth is not one); then model,
    optimizer (when the file has `optimizer` and `epoch`: args.start_epoch = epoch + 1), the average (when a model_ema is handed
    in and the file has one), the stochastic-depth seed base and the step's ``calls`` / ``skipped`` are loaded.  URLs are refused:
    this project has no network path.  The file is this project's own pickle (it holds ``args``) -- load only what you wrote."""
    import glob
    if args.auto_resume and len(args.resume) == 0:
        latest_ckpt = -1
        for ckpt in glob.glob(os.path.join(args.output_dir, "checkpoint-*.pth")):
            t = ckpt.split("-")[-1].split(".")[0]
            if t.isdigit():
                latest_ckpt = max(int(t), latest_ckpt)
        if latest_ckpt >= 0:
            args.resume = os.path.join(args.output_dir, "checkpoint-%d.pth" % latest_ckpt)
    if not args.resume:
        return
    if re.match(r"^[a-zA-Z][a-zA-Z0-9+.-]*://", args.resume):
        raise ValueError(f"auto_load_model: {args.resume!r} is a URL; only local files are loaded")
    checkpoint = torch.load(args.resume, map_location="cpu", weights_only=False)
    model.load_state_dict(checkpoint["model"])
    if "optimizer" in checkpoint and "epoch" in checkpoint:
        optimizer.load_state_dict(checkpoint["optimizer"])
        args.start_epoch = checkpoint["epoch"] + 1
        if model_ema is not None and "model_ema" in checkpoint:
            model_ema.load_state_dict(checkpoint["model_ema"])
        if "drop_seed_base" in checkpoint:
            model.engine.set_drop_seed_base(checkpoint["drop_seed_base"])
        if step is not None:
            step.calls = int(checkpoint.get("calls", 0))
            step.skipped.fill_(int(checkpoint.get("skipped", 0)))
