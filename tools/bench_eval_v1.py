#!/usr/bin/env python3
"""The v1 multi-view test on the GPU (dev tool): `tvts_amd.downstream.evaluate_v1.final_test` on ViT-B/16 with 16 frames at
224 x 224, 174 classes, 2 x 3 test views per video cut from uint8 source clips of 32 frames at 224 x 298 -- videos/s and uploaded
bytes per video.  Random weights, random clips from a seed; nothing of the reference is read.  (tools/bench_eval.py is the
pretraining side's validation bench, rows N1 - N3.)

Rows, each over the same `--batches` batches of `--videos` videos, every batch starting from HOST memory (pinned buffers) as a
loader's batch does, so the upload is inside the timed window; three alternating rounds:
    views   final_test(views=TestViews(...), file=None, merger=m) + m.result(): the uint8 source clips are shipped, the six views of
            a video are formed inside the gather, logits, ranks and the per-video sums stay on the device.
    fp32    what the package offered before: the host slices and normalises the six fp32 views of every video
            ([6, 3, 16, 224, 224] per video, the reference's ClipToTensor + Normalize as torch operations), model.forward on each
            batch of views, the logits pulled to the host for top-1 / top-5 and for the per-video mean.  Timed twice: from views
            that lie READY in pinned memory (upload + forward + host metrics: a loader whose workers hide the slicing), and IN LINE
            with the host slicing inside the window.
The gather's own time: device events around 50 launches of tvts_patch_gather_tube_u8_view on one batch's shapes, next to
tvts_patch_gather_tube_u8 on the same number of resident uint8 views, in a pass of its own.  One JSON line per round and one for
the gathers.  Timing: a host clock around `--passes` whole passes over the batches (every pass a complete final_test with a fresh
merger) that end in a device synchronise, after one warm-up pass of each row."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

KW = dict(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12, num_frames=16, tubelet_size=2)
TSRC, H0, W0 = 32, 224, 298
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def host_views(frames, plan, out):
    """uint8 [Bs, Tsrc, H0, W0, 3] -> out fp32 [B, 3, T, img, img] (pinned): slice, ClipToTensor (/ 255), Normalize, on the host"""
    mean, std = torch.tensor(MEAN).view(3, 1, 1, 1), torch.tensor(STD).view(3, 1, 1, 1)
    img = KW["img_size"]
    for b, row in enumerate(plan.view_i):
        src, t0, tstep, top, left = (int(v) for v in row[:5])
        v = frames[src, t0::tstep][:plan.T, top:top + img, left:left + img]          # [T, img, img, 3]
        out[b].copy_(v.permute(3, 0, 1, 2).float().div_(255).sub_(mean).div_(std))
    return out


def gather_us(fn, reps=50):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8, help="source clips per batch (x 6 views per forward)")
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--classes", type=int, default=174)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=8, help="passes over the batches inside one timed window")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_eval_v1.py needs an MI355X"
    from tvts_amd import hip as K
    from tvts_amd.downstream import evaluate_v1 as E
    from tvts_amd.downstream.video_encoder_v1 import VisionTransformer
    m = VisionTransformer(num_classes=args.classes, init_seed=1, **KW)
    dev = m.store.device
    views = E.TestViews(KW["img_size"], KW["img_size"], 2, 3)
    Bs, nb, V, img = args.videos, args.batches, views.per_video, KW["img_size"]
    plan = views.plan(Bs, TSRC, H0, W0)
    B, T = len(plan), plan.T
    g = torch.Generator().manual_seed(1)
    src = [torch.randint(0, 256, (Bs, TSRC, H0, W0, 3), generator=g, dtype=torch.uint8).pin_memory() for _ in range(nb)]
    target = [torch.randint(0, args.classes, (Bs,), generator=g) for _ in range(nb)]
    ids = [["v%d_%d" % (i, j) for j in range(Bs)] for i in range(nb)]
    ready = [host_views(src[i], plan, torch.empty(B, 3, T, img, img).pin_memory()) for i in range(nb)]
    inline_buf = torch.empty(B, 3, T, img, img).pin_memory()
    view_labels = [t[torch.from_numpy(plan.video.astype(np.int64))] for t in target]

    def row_views():
        merger = E.ViewMerger(nb * Bs, V, args.classes, dev, num_crop=views.test_num_crop)
        stats = E.final_test(list(zip(src, target, ids)), m, None, None, views=views, merger=merger)
        return stats, merger.result()

    def row_fp32(inline):
        hits1 = hits5 = n = 0
        per_video = []
        for i in range(nb):
            clips = host_views(src[i], plan, inline_buf) if inline else ready[i]
            logits = m(clips).cpu()
            top = logits.topk(5, dim=1).indices
            ok = top == view_labels[i][:, None]
            hits1, hits5, n = hits1 + int(ok[:, 0].sum()), hits5 + int(ok.any(dim=1).sum()), n + B
            mean = logits.double().view(Bs, V, -1).mean(dim=1)
            per_video.append((mean.topk(5, dim=1).indices == target[i][:, None]))
        pv = torch.cat(per_video)
        return dict(acc1=100.0 * hits1 / n, acc5=100.0 * hits5 / n), (100.0 * float(pv[:, 0].double().mean()), 100.0 * float(pv.any(dim=1).double().mean()))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.passes):
            out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    rows = dict(views=row_views, fp32_ready=lambda: row_fp32(False), fp32_inline=lambda: row_fp32(True))
    for fn in rows.values():  # warm-up: every shape of every row
        fn()
    nvid = nb * Bs * args.passes
    bytes_views = src[0].numel() * src[0].element_size() / Bs
    bytes_fp32 = ready[0].numel() * ready[0].element_size() / Bs
    for r in range(args.rounds):
        res = {}
        for name, fn in rows.items():
            dt, (stats, merged) = timed(fn)
            res[name] = dict(videos_per_s=nvid / dt, ms_per_video=1e3 * dt / nvid, acc1=stats["acc1"], acc5=stats["acc5"],
                             video_top1=merged[0], video_top5=merged[1])
        print(json.dumps(dict(what="v1 final_test, ViT-B/16 16 frames, 2 x 3 views from uint8 [32, 224, 298, 3] source clips", round=r,
                              videos_per_batch=Bs, batches=nb, passes=args.passes, views_per_forward=B,
                              upload_MB_per_video=dict(views=bytes_views / 1e6, fp32=bytes_fp32 / 1e6), **res)))
    # the gathers alone, on one batch's shapes
    frames = src[0].to(dev)
    table = K.view_table(plan.view_i, Bs=Bs, Tsrc=TSRC, H0=H0, W0=W0, T=T, img=img, device=dev)
    tubes, ppf, p = T // KW["tubelet_size"], (img // KW["patch_size"]) ** 2, KW["patch_size"]
    keep = torch.arange(ppf, dtype=torch.int32, device=dev).repeat(B, tubes, 1).contiguous()
    cols = torch.empty(B * tubes * ppf, 3 * KW["tubelet_size"] * p * p, dtype=torch.bfloat16, device=dev)
    sliced = torch.randint(0, 256, (B, T, img, img, 3), generator=g, dtype=torch.uint8).to(dev)
    kw = dict(B=B, tubes=tubes, tubelet=KW["tubelet_size"], n=ppf, img=img, patch=p)
    print(json.dumps(dict(what="tubelet gather alone, %d views of 16 x 224 x 224" % B,
                          u8_view_us=gather_us(lambda: K.patch_gather_tube_u8_view(frames, keep, cols, table, **kw)),
                          u8_us=gather_us(lambda: K.patch_gather_tube_u8(sliced, keep, cols, **kw)))))


if __name__ == "__main__":
    main()
