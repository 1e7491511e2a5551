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
--u8: uint8 frames [B, T, 224, 224, 3] instead of the fp32 clip (with --mixup torch there is nothing to compare: refused)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

KW = dict(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12, num_frames=16, tubelet_size=2)


def make(trainable, args):
    from tvts_amd.downstream.finetune_v1 import FinetuneStep, FusedTorchAdamW, param_groups
    from tvts_amd.downstream.video_encoder_v1 import VisionTransformer
    m = VisionTransformer(num_classes=args.classes, drop_path_rate=args.drop_path, init_seed=1, **KW)
    groups = param_groups(m, 0.05, 0.75, trainable=trainable)
    opt = FusedTorchAdamW(groups, m.store, lr=1e-3, model=m)
    for g in opt.param_groups:
        g["lr"] = 1e-4 * g["lr_scale"]
    return m, FinetuneStep(m, opt, clip_grad=5.0, trainable=trainable), len(groups)


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


def run(trainable, args, clip, targets):
    from tvts_amd import hip as K
    m, step, ngroups = make(trainable, args)
    if args.mixup == "off":
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
    if trainable == "all" and args.mixup == "off":  # the instrumented pass: events around every HBM-bound launch, the drop-path family summed
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
    del m, step
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--classes", type=int, default=174)
    ap.add_argument("--drop-path", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mixup", choices=("off", "torch", "device"), default="off")
    ap.add_argument("--u8", action="store_true", help="uint8 frames [B, T, H, W, 3] instead of the fp32 clip")
    args = ap.parse_args()
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
    if args.mixup != "off":
        targets = torch.randint(0, args.classes, (args.batch,), generator=g)  # (host labels, as a loader hands them over)
        out["mixup"] = args.mixup
    for trainable in ("all", "head") if args.mixup == "off" else ("all",):
        out["trainable=" + trainable] = run(trainable, args, clip, targets)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
