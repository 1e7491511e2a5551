#!/usr/bin/env python3
"""The v1 fine-tuning step on the GPU (dev tool): `tvts_amd.downstream.finetune_v1.FinetuneStep` on ViT-B/16 with 16 frames at
224 x 224 (S = 1569 token rows per clip), 174 classes, drop-path 0.1, layer decay 0.75 (28 parameter groups), clip_grad 5 --
clips/s for trainable = "all" (fine-tuning) and "head" (linear probing), and the share of the fine-tuning step spent in
tvts_drop_path_rows.  Random weights, random clips from a seed, soft targets; nothing of the reference is read.

Timing: the step's wall time is a host clock around `--iters` steps that end in a device synchronise, after `--warmup` steps of
the same shapes.  The drop-path figure comes from a SEPARATE pass of the same steps with HIP events around every launch of the
family (tvts_amd.hip.HBM_PROFILE, as bench.py's instrumented step does); its per-step sum is divided by the un-instrumented step
time.  One JSON line.

--mixup {off,torch,device} (default off: the run and its output as before).  Both other settings train on integer labels under
the default recipe's Mixup (mixup 0.8, cutmix 1.0, batch mode, smoothing 0.1), one plan per step drawn on the host from a fixed
seed, trainable = "all" only:
    torch   the reference's own operations (mixup.py:18-23,196-199) as torch launches on the device clip in front of the step
            -- flip, mul_, mul_, add_ (or the box copy) and the four-launch soft targets --, the step taking the mixed clip and the
            soft targets.  The clip is mixed IN PLACE step after step, as the reference mixes the loader's batch: the values drift
            towards the batch mean, the work per step does not change.
    device  step(clip, labels, mix=plan): the mix inside the gather, tvts_mix_targets.
--u8: uint8 frames [B, T, 224, 224, 3] instead of the fp32 clip (with --mixup torch there is nothing to compare: refused).

--aug {off,torch,device} (default off) with --num-sample N: the per-sample augmentation behind RandAugment (ssv2.py:186-227: random-
resized crop, flip off as for SSv2, random erasing 0.25 / pixel), one plan per step drawn on the host from a fixed seed for
B / N decoded clips of 256 x 320 and N views each, integer labels, trainable = "all" only.  Both settings start from HOST memory
every step, as a loader's batch does (pinned buffers), so the upload is inside the timed step:
    torch   the reference's torch operations on the host's normalised fp32 source clips -- slice, interpolate(bilinear), flip,
            normal_() into the erase box -- written into a pinned fp32 [B, 3, T, 224, 224] buffer, the step taking that clip.
            A second timed loop ships the already augmented pinned clip (upload + step only: a loader whose workers hide the
            augmentation); the host operations' own clock is reported too (they overlap the previous step's device work, so
            their time cannot be subtracted from the first figure).
    device  step(frames_u8, labels, aug=plan): the uint8 source frames [B / N, T, 256, 320, 3] and the plan are shipped, the gather
            does the rest.
--randaug {off,device,host} (default off; with --aug device): RandAugment rand-m7-n4-mstd0.5-inc1, bicubic, in front of the crop
(ssv2.py:174-184), drawn on the host per view from the same fixed seed:
    device  Augment(..., randaug=...): the plan carries the ops, the step runs them on the uploaded source frames
            (tvts_randaug_hist / tvts_randaug_apply) and the views of a clip still share ONE upload.  The launches' own time is
            measured too, by op class (point, blend, statistics, sharpness, bilinear, bicubic): device events around 20 launches
            of a one-layer plan in which every view has an op of that class, on the step's shapes.
    host    the same ops by PIL on the host, per view and frame, in front of the step; every view is then a uint8 clip of its own
            and is uploaded separately (B clips instead of B / N).  PIL's own clock is reported.  Without PIL: says so and skips.
--mixup device / torch may be combined with the --aug setting of the same name.  With --u8 (--aug off) or --aug device the
gather's own time is measured too: device events around 50 launches of the step's gather on the step's shapes, in a pass of its own.

--ema {off,fused,separate} (default off: the run and its output as before; without --mixup / --aug / --gpus): averaged weights,
ModelEma(decay 0.9999).
    fused     FinetuneStep(..., model_ema=ema): the average rides in the optimizer's launch (tvts_adamw_torch with ema, 38 B per element)
    separate  the step without an average, then ema.update(model) behind every call, as the reference's loop does (one more
              launch, tvts_ema_update, 12 B per element)

--opt {adamw,sgd} (default adamw: the run and its output as before; without --mixup / --aug / --gpus / --ema).  sgd: the linear-probe
script's optimizer, FusedTorchSGD (torch.optim.SGD, momentum 0.9, Nesterov: tvts_sgd_torch, 22 B per trained element against
AdamW's 30), beside FusedTorchAdamW in the SAME process: three rounds, each timing trainable = "all" and "head" under AdamW and
then under SGD (probe: lr 0.1, weight_decay 1e-9 as v1/scripts/linear_ssv2.sh; fine-tuning: lr 1e-3 x layer scale, weight_decay
0.05).  The line's "summary" gives, per setting, the SGD step over the AdamW step of the same round beside the spread of the
AdamW rounds (max / min - 1): a difference inside that spread is not a measured difference.

--guard {off,on,both} (default off: the run and its output as before; the plain step only).  on: FinetuneStep(skip_nonfinite=True),
the overflow guard (tvts_adamw_torch with skipped: one more single-lane launch, one uniform load and a branch per chunk).  both: the
guarded beside the unguarded step in the SAME process, three rounds, each timing trainable = "all" and "head" without and then
with the guard; the line's "summary" gives the guarded step over the unguarded step of the same round beside the spread of the
unguarded rounds (max / min - 1): a difference inside that spread is not a measured difference.

--gpus N: the data-parallel step, one process per GPU -- `python -m torch.distributed.run --nproc-per-node N tools/bench_finetune.py
--gpus N --batch 8 --num-sample 2` (N = 1 also runs as a plain process, without a process group).  Every rank runs the default
recipe's step on its own --batch samples (--aug device, --mixup device, --randaug device; per-rank draws seeded seed + rank as the
script does) twice in the same process: FinetuneStep with the gradient exchange, and FinetuneStep(data_parallel=False).  Rank 0
prints one JSON line: clips/s per node (N * batch over the slowest rank's step), bytes_sent per rank and updating step, both step
times and the share of the step the exchange costs, and whether the replicas' checksums agree after the run.  --payload bf16
halves the bytes.  --one-gpu: every rank on GPU 0 over gloo (the form of tools/dist_finetune_smoke.py) -- bytes_sent and the
checksum agreement only; its times say nothing about scaling and the line says so."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

KW = dict(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12, num_frames=16, tubelet_size=2)


def make(trainable, args, **step_kw):
    from tvts_amd.downstream.finetune_v1 import FinetuneStep, FusedTorchAdamW, param_groups
    from tvts_amd.downstream.video_encoder_v1 import VisionTransformer
    m = VisionTransformer(num_classes=args.classes, drop_path_rate=args.drop_path, init_seed=1, **KW)
    if getattr(args, "opt_kind", "adamw") == "sgd":
        from tvts_amd.downstream.finetune_v1 import FusedTorchSGD
        lr, wd = (0.1, 1e-9) if trainable == "head" else (1e-3, 0.05)
        groups = param_groups(m, wd, 0.75, trainable=trainable)
        opt = FusedTorchSGD(groups, m.store, lr=lr, momentum=0.9, nesterov=True, model=m)
    else:
        lr = 1e-4
        groups = param_groups(m, 0.05, 0.75, trainable=trainable)
        opt = FusedTorchAdamW(groups, m.store, lr=1e-3, model=m)
    for g in opt.param_groups:
        g["lr"] = lr * g["lr_scale"]
    ema = getattr(args, "ema", "off")
    if ema != "off":
        from tvts_amd.downstream.finetune_v1 import ModelEma
        args.model_ema = ModelEma(m, decay=0.9999)
        if ema == "fused":
            step_kw["model_ema"] = args.model_ema
    if getattr(args, "guard_on", False):
        step_kw["skip_nonfinite"] = True
    return m, FinetuneStep(m, opt, clip_grad=5.0, trainable=trainable, **step_kw), len(groups)


def torch_mix(x, labels, plan, classes):
    """the reference's Mixup.__call__ in batch mode with the plan's numbers, as torch operations on the device -> soft targets"""
    mode, (yl, yh, xl, xh) = int(plan.mix_i[0, 1]), (int(v) for v in plan.mix_i[0, 2:])
    lam, oml = float(plan.mix_f[0, 0]), float(plan.mix_f[0, 1])
    if mode == 1:
        x_flipped = x.flip(0).mul_(oml)
        x.mul_(lam).add_(x_flipped)
    elif mode == 2:
        x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]
    off = plan.smoothing / classes
    on = 1. - plan.smoothing + off
    idx = labels.to(x.device).view(-1, 1)
    y1 = torch.full((idx.shape[0], classes), off, device=x.device).scatter_(1, idx, on)
    y2 = torch.full((idx.shape[0], classes), off, device=x.device).scatter_(1, idx.flip(0), on)
    return y1 * lam + y2 * oml


SRC = (256, 320)  # the decoded clip in front of the crop (short side 256, ssv2.py:147)


def torch_aug(src, plan, img, buf):
    """the reference's torch operations (video_transforms.py:567-573,177; random_erasing.py:138-148) with the plan's numbers, on
    the host: src fp32 [Bs, 3, T, H0, W0] normalised -> buf fp32 [B, 3, T, img, img] (pinned)"""
    for b, row in enumerate(plan.aug_i):
        s_, i, j, h, w, flip, emode, et, el, eh, ew = (int(v) for v in row[:11])
        x = torch.nn.functional.interpolate(src[s_][:, :, i:i + h, j:j + w], size=(img, img), mode="bilinear", align_corners=False)
        if flip:
            x = x.flip((-1))
        if emode:
            for t in range(x.shape[1]):
                x[:, t, et:et + eh, el:el + ew] = torch.empty((3, eh, ew)).normal_()
        buf[b].copy_(x)
    return buf


RANDAUG = "rand-m7-n4-mstd0.5-inc1"
RA_CLASSES = {"point (invert)": ("invert", None), "blend (color)": ("color", 1.63), "statistics (autocontrast)": ("auto_contrast", None),
              "statistics (equalize)": ("equalize", None), "sharpness": ("sharpness", 1.63), "bilinear (rotate)": ("rotate", 21.0),
              "bicubic (rotate)": ("rotate", 21.0)}


def pil_op(im, fn, arg, resample):
    """one RandAugment op of a plan's record on a PIL image, as PIL's own calls"""
    from PIL import Image, ImageEnhance, ImageOps
    fill = dict(fillcolor=(128, 128, 128), resample=resample)
    if fn == "auto_contrast":
        return ImageOps.autocontrast(im)
    if fn == "equalize":
        return ImageOps.equalize(im)
    if fn == "invert":
        return ImageOps.invert(im)
    if fn == "solarize":
        return ImageOps.solarize(im, arg)
    if fn == "solarize_add":
        return im.point([min(255, i + arg) if i < 128 else i for i in range(256)] * 3)
    if fn == "posterize":
        return im if arg >= 8 else ImageOps.posterize(im, arg)
    if fn in ("color", "contrast", "brightness", "sharpness"):
        return getattr(ImageEnhance, fn.capitalize())(im).enhance(arg)
    if fn == "rotate":
        return im.rotate(arg, **fill)
    w, h = im.size
    data = {"shear_x": (1, arg, 0, 0, 1, 0), "shear_y": (1, 0, 0, arg, 1, 0), "translate_x_rel": (1, 0, arg * w, 0, 1, 0),
            "translate_y_rel": (1, 0, 0, 0, 1, arg * h)}[fn]
    return im.transform(im.size, Image.AFFINE, data, **fill)


def randaug_class_us(frames, Bs, B, ns, reps=20):
    """device events around the hist and apply launches of one-layer plans, every view an op of one class -> {class: us}"""
    from tvts_amd import hip as K
    from tvts_amd.downstream.finetune_v1 import ra_plan, ra_row
    work = torch.empty((Bs + 2 * B,) + tuple(frames.shape[1:]), dtype=torch.uint8, device="cuda")
    work[:Bs].copy_(frames)
    H0, W0 = frames.shape[2], frames.shape[3]
    hist = torch.empty((B, frames.shape[1], 4, 256), dtype=torch.int32, device="cuda")
    lib, p, st = K._lib.load(), K._p, K._stream
    out = {}
    for name, (fn, arg) in RA_CLASSES.items():
        row = ra_row(fn, arg, 2 if "bilinear" in name else 3, H0, W0)
        plan = ra_plan([([row], [])] * B, 1, ns)
        t = K.RandaugTable(plan.ra_i, plan.ra_d, Bs=Bs, num_sample=ns)
        a = (p(work), Bs, B, ns, frames.shape[1], H0, W0, 0, 1, p(t.ra_i))
        if t.stats[0]:
            out[name + ": hist us"] = gather_us(lambda: lib.tvts_randaug_hist(*a, p(hist), st()), reps)
        out[name + ": apply us"] = gather_us(lambda: lib.tvts_randaug_apply(*a, p(t.ra_d), p(hist) if t.stats[0] else None, st()), reps)
    out["bytes read + written per apply launch"] = 2 * B * frames[0].numel()
    return out


def gather_us(fn, reps=50):
    """device events around `reps` launches of the step's gather (all patches kept) -> microseconds per launch"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def run_aug(args, targets):
    """--aug torch / device -> the result dict of trainable = "all" """
    import random

    import numpy as np
    from tvts_amd import hip as K
    from tvts_amd.downstream.finetune_v1 import AugPlan, Augment, Mixup, RandAugment
    m, step, ngroups = make("all", args)
    img, T, B, Bs = KW["img_size"], KW["num_frames"], args.batch, args.batch // args.num_sample
    random.seed(0)
    np.random.seed(0)
    aug = Augment(img, hflip=0.0, reprob=0.25, remode="pixel", recount=1, num_sample=args.num_sample,
                  randaug=None if args.randaug == "off" else RandAugment(RANDAUG, interpolation="bicubic", input_size=img))
    mixup = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1, num_classes=args.classes)
    g = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (Bs, T, SRC[0], SRC[1], 3), generator=g, dtype=torch.uint8).pin_memory()
    host = dict(s=0.0)
    if args.randaug == "host":
        from PIL import Image
        views = torch.empty((B, T, SRC[0], SRC[1], 3), dtype=torch.uint8).pin_memory()
        src_np, views_np = frames.numpy(), views.numpy()

        def one():
            plan = aug.draw(Bs, *SRC)
            t0 = time.perf_counter()
            for b, ops in enumerate(plan.ra.ops):
                for t in range(T):
                    im = Image.fromarray(src_np[b // args.num_sample, t])
                    for fn, arg, rs in ops:
                        im = pil_op(im, fn, arg, rs)
                    views_np[b, t] = np.asarray(im)
            host["s"] += time.perf_counter() - t0
            own = plan.aug_i.copy()
            own[:, 0] = np.arange(B)  # every view is a source clip of its own
            return step.step(views, targets, aug=AugPlan(own), mix=mixup.draw(B, img) if args.mixup == "device" else None)
    elif args.aug == "device":
        def one():
            plan = aug.draw(Bs, *SRC)
            return step.step(frames, targets, aug=plan, mix=mixup.draw(B, img) if args.mixup == "device" else None)
    else:
        mean, std = torch.tensor(K.IMAGENET_MEAN).view(1, 1, 1, 1, 3), torch.tensor(K.IMAGENET_STD).view(1, 1, 1, 1, 3)
        src = ((frames.float() / 255.0 - mean) / std).permute(0, 4, 1, 2, 3).contiguous()
        buf = torch.empty(B, 3, T, img, img).pin_memory()

        def one():
            t0 = time.perf_counter()
            clip = torch_aug(src, aug.draw(Bs, *SRC), img, buf)
            host["s"] += time.perf_counter() - t0
            if args.mixup == "torch":
                clip = clip.cuda()
                return step.step(clip, torch_mix(clip, targets, mixup.draw(B, img), args.classes))
            return step.step(clip, targets)
    for _ in range(args.warmup):
        out = one()
    torch.cuda.synchronize()
    host["s"] = 0.0
    t0 = time.perf_counter()
    for _ in range(args.iters):
        out = one()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.iters
    res = {"step ms": 1e3 * dt, "clips/s": B / dt, "parameter groups": ngroups, "last loss": float(out["loss"]),
           "upload bytes/step": (frames if args.aug == "device" else buf).numel() * (1 if args.aug == "device" else 4)}
    if args.randaug == "host":
        res.update({"upload bytes/step": views.numel(), "host RandAugment (PIL) ms/step": 1e3 * host["s"] / args.iters})
    if args.randaug == "device":
        res["randaug launches by op class (events, 20 launches)"] = randaug_class_us(frames, Bs, B, args.num_sample)
    if args.aug == "torch":
        res["host augment ms/step"] = 1e3 * host["s"] / args.iters
        if args.mixup == "off":  # upload + step only, from the pinned buffer the last step left
            for _ in range(args.warmup):
                step.step(buf, targets)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                step.step(buf, targets)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.iters
            res.update({"step ms, augmented clip ready on the host": 1e3 * dt, "clips/s, augmented clip ready on the host": B / dt})
    else:
        a, eng = m.engine.arch, m.engine
        tubes, ppf, kc = T // a["tubelet"], (img // a["patch"]) ** 2, 3 * a["tubelet"] * a["patch"] ** 2
        keep = torch.arange(ppf, dtype=torch.int32, device="cuda").repeat(B, tubes, 1).contiguous()
        cols = torch.empty(B * tubes * ppf, kc, dtype=torch.bfloat16, device="cuda")
        plan = Augment(img, hflip=0.0, reprob=0.25, remode="pixel", recount=1, num_sample=args.num_sample).draw(Bs, *SRC)
        table, fr = K.aug_table(plan.aug_i, Bs=Bs, H0=SRC[0], W0=SRC[1], img=img), frames.cuda()
        kw = dict(B=B, tubes=tubes, tubelet=a["tubelet"], n=ppf, img=img, patch=a["patch"])
        crop_bytes = int(sum(int(r[3]) * int(r[4]) for r in plan.aug_i)) * 3 * T
        res.update({"gather us (events, 50 launches)": gather_us(lambda: K.patch_gather_tube_u8_aug(fr, keep, cols, table, None, **kw)),
                    "gather bytes (crop source + 2 B per output element)": crop_bytes + 2 * cols.numel()})
        ident = plan.aug_i.copy()
        ident[:, 1:11] = (16, 48, img, img, 0, 0, 0, 0, 0, 0)
        table = K.aug_table(ident, Bs=Bs, H0=SRC[0], W0=SRC[1], img=img)
        res["gather us, identity crops, no erase"] = gather_us(lambda: K.patch_gather_tube_u8_aug(fr, keep, cols, table, None, **kw))
        crop = torch.tensor([[16, 48]] * Bs, dtype=torch.int32, device="cuda")
        kw["B"], keep, cols = Bs, keep[:Bs].contiguous(), cols[:Bs * tubes * ppf]
        res["plain u8 gather us on the source clips (B / N samples)"] = gather_us(
            lambda: K.patch_gather_tube_u8(fr, keep, cols, crop=crop, **kw))
    del m, step
    torch.cuda.empty_cache()
    return res


def run(trainable, args, clip, targets):
    from tvts_amd import hip as K
    m, step, ngroups = make(trainable, args)
    if args.ema == "separate":
        def one():
            out = step.step(clip, targets)
            args.model_ema.update(m)
            return out
    elif args.mixup == "off":
        one = lambda: step.step(clip, targets)
    else:
        import numpy as np
        from tvts_amd.downstream.finetune_v1 import Mixup
        np.random.seed(0)
        fn = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1, num_classes=args.classes)
        img = KW["img_size"]
        if args.mixup == "device":
            one = lambda: step.step(clip, targets, mix=fn.draw(args.batch, img))
        else:
            one = lambda: step.step(clip, torch_mix(clip, targets, fn.draw(args.batch, img), args.classes))
    for _ in range(args.warmup):
        out = one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        out = one()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.iters
    res = {"step ms": 1e3 * dt, "clips/s": args.batch / dt, "parameter groups": ngroups, "last loss": float(out["loss"])}
    if trainable == "all" and args.mixup == "off" and args.opt == "adamw":  # the instrumented pass: events around every HBM-bound launch, the drop-path family summed
        reps = max(2, args.iters // 4)
        K.HBM_PROFILE = []
        try:
            for _ in range(reps):
                step.step(clip, targets)
            torch.cuda.synchronize()
            ms = sum(e0.elapsed_ms(e1) for fam, _, e0, e1 in K.HBM_PROFILE if fam == "drop_path")
            n = sum(1 for fam, *_ in K.HBM_PROFILE if fam == "drop_path")
        finally:
            K.HBM_PROFILE = None
        res.update({"drop_path_rows launches/step": n / reps, "drop_path_rows ms/step (events)": ms / reps,
                    "drop_path_rows share of the step": ms / reps / (1e3 * dt)})
    if trainable == "all" and clip.dtype == torch.uint8:  # the uint8 gather's own time, on the step's shapes
        a, B = m.engine.arch, clip.shape[0]
        tubes, ppf, kc = clip.shape[1] // a["tubelet"], (a["image"] // a["patch"]) ** 2, 3 * a["tubelet"] * a["patch"] ** 2
        keep = torch.arange(ppf, dtype=torch.int32, device="cuda").repeat(B, tubes, 1).contiguous()
        cols = torch.empty(B * tubes * ppf, kc, dtype=torch.bfloat16, device="cuda")
        res["gather us (events, 50 launches)"] = gather_us(lambda: K.patch_gather_tube_u8(
            clip, keep, cols, B=B, tubes=tubes, tubelet=a["tubelet"], n=ppf, img=a["image"], patch=a["patch"]))
        res["gather bytes (source + 2 B per output element)"] = clip.numel() + 2 * cols.numel()
    del m, step
    torch.cuda.empty_cache()
    return res


def run_dist(args):
    """--gpus N -> one JSON line on rank 0 (see the module docstring)"""
    import random

    import numpy as np
    import torch.distributed as dist
    from tvts_amd import dist as D
    from tvts_amd.downstream.finetune_v1 import Augment, Mixup, RandAugment
    launched = "WORLD_SIZE" in os.environ
    if args.gpus > 1 and not launched:
        raise SystemExit(f"--gpus {args.gpus}: run under `python -m torch.distributed.run --nproc-per-node {args.gpus}`")
    if launched:
        if int(os.environ["WORLD_SIZE"]) != args.gpus:
            raise SystemExit(f"--gpus {args.gpus} under a launcher with WORLD_SIZE={os.environ['WORLD_SIZE']}")
        torch.cuda.set_device(0 if args.one_gpu else int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("gloo" if args.one_gpu else "nccl")
    W, rank = D.world()
    dev = torch.cuda.current_device()
    img, T, B, Bs = KW["img_size"], KW["num_frames"], args.batch, args.batch // args.num_sample
    frames = torch.randint(0, 256, (Bs, T, SRC[0], SRC[1], 3), generator=torch.Generator().manual_seed(1 + rank), dtype=torch.uint8).pin_memory()
    labels = torch.randint(0, args.classes, (B,), generator=torch.Generator().manual_seed(100 + rank))
    res = {}
    for name, dp in (("exchange", None), ("data_parallel=False", False)):
        random.seed(rank)
        np.random.seed(rank)
        aug = Augment(img, hflip=0.0, reprob=0.25, remode="pixel", recount=1, num_sample=args.num_sample,
                      randaug=RandAugment(RANDAUG, interpolation="bicubic", input_size=img))
        mixup = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.1, num_classes=args.classes)
        m, step, _ = make("all", args, data_parallel=dp, payload=args.payload)

        def one():
            return step.step(frames, labels, aug=aug.draw(Bs, *SRC), mix=mixup.draw(B, img))
        for _ in range(args.warmup):
            one()
        torch.cuda.synchronize()
        if W > 1:
            dist.barrier()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            out = one()
        torch.cuda.synchronize()
        res[name] = dict(ms=1e3 * (time.perf_counter() - t0) / args.iters, bytes=step.bytes_sent, loss=float(out["loss"]),
                         checksum=int(step.replicas_checksum()) if dp is None else 0)
        del m, step
        torch.cuda.empty_cache()
    ex, loc = res["exchange"], res["data_parallel=False"]
    # (the checksum travels as two 31-bit halves: gather_rows sums in float64-exact integers either way, this keeps it readable)
    row = torch.tensor([ex["ms"], loc["ms"], float(ex["bytes"]), float(ex["checksum"] & 0x7FFFFFFF), float((ex["checksum"] >> 31) & 0x7FFFFFFF)],
                       dtype=torch.float64)
    rows = D.gather_rows(row)
    if W > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank != 0:
        return
    slow_ex, slow_loc = float(rows[:, 0].max()), float(rows[:, 1].max())
    out = {"what": "v1 FinetuneStep across ranks, ViT-B/16, 16 frames at 224, default recipe (aug, RandAugment, Mixup on the device)",
           "gpus": W, "batch per rank": B, "num_sample": args.num_sample, "payload": args.payload or os.environ.get("TVTS_GRAD_PAYLOAD", "fp32"),
           "transport": D.transport() if W > 1 else "none", "backend": ("gloo, every rank on GPU 0" if args.one_gpu else "nccl") if W > 1 else "none",
           "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(dev),
           "step ms with the exchange (slowest rank)": slow_ex, "step ms, data_parallel=False (slowest rank)": slow_loc,
           "exchange share of the step": (slow_ex - slow_loc) / slow_ex, "clips/s per node": W * B / (1e-3 * slow_ex),
           "bytes_sent per rank and step": int(rows[0, 2]), "step ms by rank": [round(float(v), 3) for v in rows[:, 0]],
           "replicas' checksums agree": bool((rows[:, 3:] == rows[0, 3:]).all()), "last loss (rank 0)": ex["loss"]}
    if args.one_gpu and W > 1:
        out["scaling"] = "NOT MEASURED: the ranks share one GPU (times above are not a scaling figure)"
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=0, help="the data-parallel step on N ranks (under torch.distributed.run); see the docstring")
    ap.add_argument("--one-gpu", action="store_true", help="with --gpus N: every rank on GPU 0 over gloo (bytes and correctness only)")
    ap.add_argument("--payload", choices=("fp32", "bf16"), default=None, help="with --gpus N: the gradients' format on the links")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--classes", type=int, default=174)
    ap.add_argument("--drop-path", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mixup", choices=("off", "torch", "device"), default="off")
    ap.add_argument("--u8", action="store_true", help="uint8 frames [B, T, H, W, 3] instead of the fp32 clip")
    ap.add_argument("--aug", choices=("off", "torch", "device"), default="off")
    ap.add_argument("--num-sample", type=int, default=1, help="views per decoded clip (--num_sample of the script)")
    ap.add_argument("--randaug", choices=("off", "device", "host"), default="off", help="RandAugment in front of the crop (--aug device)")
    ap.add_argument("--ema", choices=("off", "fused", "separate"), default="off", help="ModelEma: in the optimizer's launch, or update() behind the step")
    ap.add_argument("--opt", choices=("adamw", "sgd"), default="adamw", help="sgd: FusedTorchSGD beside FusedTorchAdamW in the same run, three rounds")
    ap.add_argument("--guard", choices=("off", "on", "both"), default="off", help="skip_nonfinite: on, or both: guarded beside unguarded, three rounds")
    args = ap.parse_args()
    if args.guard != "off" and (args.gpus or args.mixup != "off" or args.aug != "off" or args.ema != "off" or args.u8 or args.opt != "adamw"):
        raise SystemExit("--guard on / both: the plain step only (without --gpus, --mixup, --aug, --ema, --u8, --opt sgd)")
    args.guard_on = args.guard == "on"
    if args.opt != "adamw" and (args.gpus or args.mixup != "off" or args.aug != "off" or args.ema != "off" or args.u8):
        raise SystemExit("--opt sgd: the plain step only (without --gpus, --mixup, --aug, --ema, --u8)")
    if args.ema != "off" and (args.gpus or args.mixup != "off" or args.aug != "off"):
        raise SystemExit("--ema fused / separate: the plain step only (without --gpus, --mixup, --aug)")
    if args.gpus:
        if args.gpus < 1 or args.batch % 2 or args.num_sample < 1 or args.batch % args.num_sample:
            raise SystemExit("--gpus N >= 1, an even --batch (Mixup) and --num-sample a divisor of it")
        if not torch.cuda.is_available():
            raise SystemExit("bench_finetune.py measures on the GPU; there is none here (NOT MEASURED)")
        return run_dist(args)
    if args.randaug != "off" and args.aug != "device":
        raise SystemExit("--randaug device / host: with --aug device (the rest of the augmentation stays on the device)")
    if args.randaug == "host":
        try:
            import PIL  # noqa: F401
        except ImportError:
            print("--randaug host: PIL is not importable here; skipped (NOT MEASURED)", flush=True)
            return
    if args.aug != "off" and (args.u8 or args.mixup not in ("off", args.aug)):
        raise SystemExit("--aug torch / device: without --u8 (the setting says what is shipped), --mixup off or the same setting")
    if args.num_sample < 1 or args.batch % args.num_sample or (args.aug == "off" and args.num_sample != 1):
        raise SystemExit("--num-sample: a divisor of --batch, with --aug torch / device")
    if args.u8 and args.mixup == "torch":
        raise SystemExit("--u8 --mixup torch: the reference mixes normalised fp32 clips, there is no torch form on uint8 frames")
    if args.mixup != "off" and args.batch % 2:
        raise SystemExit("--mixup needs an even --batch")
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune.py measures on the GPU; there is none here (NOT MEASURED)")
    g = torch.Generator().manual_seed(0)
    clip = torch.randn(args.batch, 3, KW["num_frames"], KW["img_size"], KW["img_size"], generator=g).cuda()
    targets = torch.softmax(2.0 * torch.randn(args.batch, args.classes, generator=g), dim=1)
    out = {"what": "v1 FinetuneStep, ViT-B/16, 16 frames at 224 (S = 1569)", "batch": args.batch, "classes": args.classes,
           "drop_path_rate": args.drop_path, "iters": args.iters, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0)}
    if args.u8:
        clip = torch.randint(0, 256, (args.batch, KW["num_frames"], KW["img_size"], KW["img_size"], 3), generator=g, dtype=torch.uint8).cuda()
        out["input"] = "uint8 frames"
    if args.ema != "off":
        out["ema"] = args.ema
    if args.mixup != "off":
        targets = torch.randint(0, args.classes, (args.batch,), generator=g)  # (host labels, as a loader hands them over)
        out["mixup"] = args.mixup
    if args.aug != "off":
        out.update({"aug": args.aug, "num_sample": args.num_sample, "source": "%d x %d" % SRC})
        if args.randaug != "off":
            out["randaug"] = "%s (%s, bicubic)" % (args.randaug, RANDAUG)
        if args.mixup == "off":
            targets = torch.randint(0, args.classes, (args.batch,), generator=g)
        out["trainable=all"] = run_aug(args, targets)
        print(json.dumps(out), flush=True)
        return
    if args.opt == "sgd":
        rounds = []
        for _ in range(3):
            rnd = {}
            for kind in ("adamw", "sgd"):
                args.opt_kind = kind
                rnd[kind] = {"trainable=" + t: run(t, args, clip, targets) for t in ("all", "head")}
            rounds.append(rnd)
        out["optimizers"] = {"adamw": "FusedTorchAdamW (tvts_adamw_torch)", "sgd": "FusedTorchSGD momentum 0.9 nesterov (tvts_sgd_torch)"}
        out["rounds"] = rounds
        summary = {}
        for t in ("trainable=all", "trainable=head"):
            adam = [r["adamw"][t]["step ms"] for r in rounds]
            sgd = [r["sgd"][t]["step ms"] for r in rounds]
            summary[t] = {"adamw step ms by round": adam, "sgd step ms by round": sgd,
                          "sgd / adamw by round": [b / a for a, b in zip(adam, sgd)],
                          "spread of the adamw rounds (max / min - 1)": max(adam) / min(adam) - 1.0}
        out["summary"] = summary
        print(json.dumps(out), flush=True)
        return
    if args.guard == "both":
        rounds = []
        for _ in range(3):
            rnd = {}
            for kind in ("off", "on"):
                args.guard_on = kind == "on"
                rnd[kind] = {"trainable=" + t: run(t, args, clip, targets) for t in ("all", "head")}
            rounds.append(rnd)
        out["guard"] = {"off": "FinetuneStep (tvts_adamw_torch)", "on": "FinetuneStep(skip_nonfinite=True) (tvts_adamw_torch with skipped)"}
        out["rounds"] = rounds
        summary = {}
        for t in ("trainable=all", "trainable=head"):
            off = [r["off"][t]["step ms"] for r in rounds]
            on = [r["on"][t]["step ms"] for r in rounds]
            summary[t] = {"unguarded step ms by round": off, "guarded step ms by round": on,
                          "guarded / unguarded by round": [b / a for a, b in zip(off, on)],
                          "spread of the unguarded rounds (max / min - 1)": max(off) / min(off) - 1.0}
        out["summary"] = summary
        print(json.dumps(out), flush=True)
        return
    if args.guard == "on":
        out["guard"] = "on"
    for trainable in ("all", "head") if args.mixup == "off" else ("all",):
        out["trainable=" + trainable] = run(trainable, args, clip, targets)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
