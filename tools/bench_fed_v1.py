#!/usr/bin/env python3
"""The v1 pretraining step fed from PINNED HOST memory every iteration, per wire format of EngineV1.prepare_batch (bench.py times
batches that are resident in HBM).  README's v1 configuration: 4 frames, 256 clips, 224^2.  Eager launches, prepare_batch (H2D copies,
descriptors, token sort) inside the timed loop.  Legs, with the bytes one step uploads at 256 x 4 frames:

    fp32        fp32 [B, T, 3, 224, 224], the parent's path and the baseline                  616 MB
    u8_crop     uint8 [B, T, 224, 224, 3], cropped on the host                                154 MB
    u8_resized  uint8 [B, T, 268, 476, 3] + crop: resized on the host, cropped on the device  392 MB
    u8_source   uint8 [B, T, 360, 640, 3] + crop + resize=268: Pillow's Resize on the device  708 MB

A fresh process per leg, the legs alternating over ROUNDS rounds; per leg the median ms per step over all its blocks, the H2D bytes
of the clip tensor, and (u8_source) the resize kernels' own time from events.  The reference-equivalent host chain (PIL resize + crop
+ ClipToTensor + Normalize) of ONE clip is timed on one core beside them: what the device takes over.  Dev tool, GPU only.

    python tools/bench_fed_v1.py [--batch 256] [--frames 4] [--rounds 3] [--out FILE.json]
    python tools/bench_fed_v1.py --leg u8_source          (one leg in this process; prints one JSON line)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("fp32", "u8_crop", "u8_resized", "u8_source")
IMG, SIZE, SRC, RESIZED = 224, 268, (360, 640), (268, 476)


def host_chain_ms(T, reps=5):
    """ms per clip of the reference's chain on one core: T frames of 360 x 640 -> PIL BILINEAR Resize(268) -> crop 224 -> fp32 / 255 ->
    Normalize (None without Pillow)"""
    try:
        from PIL import Image
    except ImportError:
        return None
    import numpy as np
    import torch
    torch.set_num_threads(1)
    frames = np.random.RandomState(0).randint(0, 256, size=(T,) + SRC + (3,), dtype=np.uint8)
    mean, std = torch.tensor([0.485, 0.456, 0.406])[:, None, None, None], torch.tensor([0.229, 0.224, 0.225])[:, None, None, None]
    best = []
    for _ in range(reps):
        t = time.perf_counter()
        pil = [Image.fromarray(f).convert("RGB") for f in frames]
        pil = [im.resize((RESIZED[1], RESIZED[0]), Image.BILINEAR) for im in pil]
        pil = [im.crop((100, 20, 100 + IMG, 20 + IMG)) for im in pil]
        clip = np.zeros([3, T, IMG, IMG])
        for i, im in enumerate(pil):
            clip[:, i] = np.asarray(im).transpose(2, 0, 1)
        x = torch.from_numpy(clip).float().div(255)
        x.sub_(mean).div_(std)
        best.append((time.perf_counter() - t) * 1e3)
    return statistics.median(best)


def run_leg(leg, B, T, blocks, steps):
    import torch

    from tvts_amd import arch as A
    from tvts_amd import hip as K
    from tvts_amd.data_loader import synth_batch_v1
    from tvts_amd.model.model_dist_TVTS import TVTS
    from tvts_amd.optim import FusedHFAdamW
    from tvts_amd.step import StepRunner

    a = dict(A.ARCHS["v1"])
    m = TVTS(types.SimpleNamespace(local_rank=0, rank=0, world_size=1), arch=a, init_seed=0)
    groups = [[], [], [], []]
    for name, p in m.named_parameters():  # (bench.py's v1 setup: one AdamW rule, lr 1e-4, no weight decay)
        gi = A.param_group_of(name, a)
        if gi < 0:
            p.requires_grad = False
        else:
            groups[gi].append(p)
    opt = FusedHFAdamW([dict(params=g, lr=1e-4, weight_decay=0.0) for g in groups if g], m.store, model=m)
    run = StepRunner(m, opt)
    m._fresh_shadows(); m._sync_requires_grad()
    pool = []
    for i in range(2):
        b = synth_batch_v1(a, B, T, seed=i, caption_len=32)
        g = torch.Generator().manual_seed(100 + i)
        if leg == "fp32":
            b["video"] = b["video"].pin_memory()
        else:
            H, W = {"u8_crop": (IMG, IMG), "u8_resized": RESIZED, "u8_source": SRC}[leg]
            b["video"] = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.uint8).pin_memory()
            if leg != "u8_crop":
                b["crop"] = torch.stack([torch.randint(0, RESIZED[0] - IMG + 1, (B,), generator=g),
                                         torch.randint(0, RESIZED[1] - IMG + 1, (B,), generator=g)], 1).to(torch.int32)
            if leg == "u8_source":
                b["resize"] = SIZE
        pool.append(b)
    labels = [b["label"].reshape(-1).to(torch.int32).to("cuda:0") for b in pool]
    events = []
    if leg == "u8_source":
        inner = K.resize_crop_u8

        def timed(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            inner(*args, **kw)
            e1.record()
            events.append((e0, e1))
        K.resize_crop_u8 = timed
    for it in range(3):
        run.run(m.engine.prepare_batch(pool[it % 2]), labels[it % 2])
    torch.cuda.synchronize()
    del events[:]
    ms = []
    for _ in range(blocks):
        t = time.perf_counter()
        for it in range(steps):
            run.run(m.engine.prepare_batch(pool[it % 2]), labels[it % 2])
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3 / steps)
    out = dict(leg=leg, B=B, T=T, ms_per_step=ms, h2d_bytes=int(pool[0]["video"].numel() * pool[0]["video"].element_size()))
    if events:
        out["resize_kernel_ms"] = statistics.median(e0.elapsed_time(e1) for e0, e1 in events)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.leg:
        print("LEG " + json.dumps(run_leg(args.leg, args.batch, args.frames, args.blocks, args.steps)), flush=True)
        return
    res = {leg: dict(ms=[], h2d_bytes=None, resize_kernel_ms=[]) for leg in LEGS}
    for rnd in range(args.rounds):
        for leg in LEGS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--batch", str(args.batch), "--frames",
                                str(args.frames), "--blocks", str(args.blocks), "--steps", str(args.steps)],
                               capture_output=True, text=True, timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")]
            if p.returncode != 0 or not line:
                print(f"round {rnd} leg {leg} failed (rc {p.returncode}):\n{p.stderr[-2000:]}", flush=True)
                sys.exit(1)  # nothing more is started on the device behind a failed leg
            r = json.loads(line[0][4:])
            res[leg]["ms"] += r["ms_per_step"]
            res[leg]["h2d_bytes"] = r["h2d_bytes"]
            if "resize_kernel_ms" in r:
                res[leg]["resize_kernel_ms"].append(r["resize_kernel_ms"])
            print(f"round {rnd} {leg:10s} {['%.2f' % v for v in r['ms_per_step']]} ms/step", flush=True)
    base = statistics.median(res["fp32"]["ms"])
    summary = dict(batch=args.batch, frames=args.frames, host_chain_ms_per_clip=host_chain_ms(args.frames), legs={})
    for leg in LEGS:
        med = statistics.median(res[leg]["ms"])
        summary["legs"][leg] = dict(median_ms=med, min_ms=min(res[leg]["ms"]), max_ms=max(res[leg]["ms"]), vs_fp32=med / base,
                                    pairs_per_s=args.batch / med * 1e3, h2d_MB=res[leg]["h2d_bytes"] / 1e6,
                                    resize_kernel_ms=statistics.median(res[leg]["resize_kernel_ms"]) if res[leg]["resize_kernel_ms"] else None)
        print(f"{leg:10s} median {med:7.2f} ms/step ({min(res[leg]['ms']):.2f} .. {max(res[leg]['ms']):.2f})  x{med / base:.3f} of fp32  "
              f"{args.batch / med * 1e3:7.1f} pairs/s  H2D {res[leg]['h2d_bytes'] / 1e6:6.1f} MB", flush=True)
    print("RESULT " + json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
