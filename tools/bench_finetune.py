#!/usr/bin/env python3
"""The v1 fine-tuning step on the GPU (dev tool): `tvts_amd.downstream.finetune_v1.FinetuneStep` on ViT-B/16 with 16 frames at
224 x 224 (S = 1569 token rows per clip), 174 classes, drop-path 0.1, layer decay 0.75 (28 parameter groups), clip_grad 5 --
clips/s for trainable = "all" (fine-tuning) and "head" (linear probing), and the share of the fine-tuning step spent in
tvts_drop_path_rows.  Random weights, random clips from a seed, soft targets; nothing of the reference is read.

Timing: the step's wall time is a host clock around `--iters` steps that end in a device synchronise, after `--warmup` steps of
the same shapes.  The drop-path figure comes from a SEPARATE pass of the same steps with HIP events around every launch of the
family (tvts_amd.hip.HBM_PROFILE, as bench.py's instrumented step does); its per-step sum is divided by the un-instrumented step
time.  One JSON line."""
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


def run(trainable, args, clip, targets):
    from tvts_amd import hip as K
    m, step, ngroups = make(trainable, args)
    for _ in range(args.warmup):
        out = step.step(clip, targets)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        out = step.step(clip, targets)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.iters
    res = {"step ms": 1e3 * dt, "clips/s": args.batch / dt, "parameter groups": ngroups, "last loss": float(out["loss"])}
    if trainable == "all":  # the instrumented pass: events around every HBM-bound launch, the drop-path family summed
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune.py measures on the GPU; there is none here (NOT MEASURED)")
    g = torch.Generator().manual_seed(0)
    clip = torch.randn(args.batch, 3, KW["num_frames"], KW["img_size"], KW["img_size"], generator=g).cuda()
    targets = torch.softmax(2.0 * torch.randn(args.batch, args.classes, generator=g), dim=1)
    out = {"what": "v1 FinetuneStep, ViT-B/16, 16 frames at 224 (S = 1569)", "batch": args.batch, "classes": args.classes,
           "drop_path_rate": args.drop_path, "iters": args.iters, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0)}
    for trainable in ("all", "head"):
        out["trainable=" + trainable] = run(trainable, args, clip, targets)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
