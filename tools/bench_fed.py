#!/usr/bin/env python3
"""The step fed from HOST memory every iteration (the trainer's situation; bench.py times inputs that are resident in HBM): eager
launches, prepare_batch (dtype / device normalisation, token sort, H2D copies) inside the timed loop.  Dev tool, GPU only.

    python tools/bench_fed.py [PAIRS]
        one process: fp32 clips as the reference's loader hands them over (pageable / pinned) and the uint8 wire format of SURVEY 8f N3

    python tools/bench_fed.py --legs [--batch 192] [--frames 8] [--rounds 3] [--out FILE.json]
        the wire formats of Engine.prepare_batch for DECODER-sized clips (DESIGN.md 8j "v2 ragged"), B/16 at 224^2, Resize(268):
            fp32            fp32 [B, T, 3, 224, 224], pinned: the host did the whole chain
            u8_uniform      uint8 [B, T, 360, 640, 3], pinned, + crop + resize: one source size (tvts_patch_gather_u8_resized)
            u8_ragged       a list of clips in three source sizes -- 360 x 640, 640 x 360 and 240 x 320 (upscaled) -- + crop + resize
                            (packed on the host, tvts_patch_gather_u8_ragged)
            u8_ragged_short the same list with a tenth of the clips short (half the frames) or failed (one black 224 x 224 frame)
        A fresh process per leg, the legs alternating over ROUNDS rounds; per leg the median and min .. max ms per step over all its
        blocks, the bytes one step uploads, the gather entry point's own time from events around it and the host's packing time.
    python tools/bench_fed.py --leg u8_ragged       (one leg in this process; prints one JSON line)
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

LEGS = ("fp32", "u8_uniform", "u8_ragged", "u8_ragged_short")
IMG, SIZE = 224, 268
SOURCES = ((360, 640), (640, 360), (240, 320))


def build(a):
    import torch  # noqa: F401

    from tvts_amd import arch as A
    from tvts_amd.model._common import TVTSv2Base
    from tvts_amd.optim import FusedHFAdamW
    from tvts_amd.step import StepRunner
    m = TVTSv2Base(types.SimpleNamespace(local_rank=0, rank=0, world_size=1), arch=a, init_seed=0)
    groups = [[], [], [], []]
    for name, p in m.named_parameters():
        gi = A.param_group_of(name, a)
        if gi < 0:
            p.requires_grad = False
        else:
            groups[gi].append(p)
    opt = FusedHFAdamW([dict(params=groups[i], lr=A.GROUP_HPARAMS[i][0], weight_decay=A.GROUP_HPARAMS[i][1]) for i in range(4)], m.store, model=m)
    run = StepRunner(m, opt)
    m._fresh_shadows(); m._sync_requires_grad()
    return m, run


def one_process(B):
    import torch

    from tvts_amd import arch as A
    from tvts_amd.data_loader import synth_batch
    a = dict(A.ARCHS["B_16"])
    m, run = build(a)
    pool = [synth_batch(a, B, 8, seed=i, caption_len=32) for i in range(2)]

    def variant(kind):
        out = []
        for b in pool:
            b = dict(b)
            if kind == "fp32 pinned":
                b["video"] = b["video"].pin_memory()
            elif kind.startswith("uint8"):
                v = (b["video"] * 40 + 128).clamp(0, 255).to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous()  # [B, T, H, W, 3] frames
                b["video"] = v.pin_memory() if "pinned" in kind else v
            out.append(b)
        return out

    for kind in ("resident", "fp32 pageable", "fp32 pinned", "uint8 pinned"):
        bs = variant(kind)
        pbs = [m.engine.prepare_batch(b) for b in bs] if kind == "resident" else None
        labs = [b["label"].reshape(-1).to(torch.int32).to("cuda:0") for b in bs]
        for it in range(3):
            run.run(pbs[it % 2] if pbs else m.engine.prepare_batch(bs[it % 2]), labs[it % 2])
        torch.cuda.synchronize()
        n = 10
        t = time.time()
        for it in range(n):
            run.run(pbs[it % 2] if pbs else m.engine.prepare_batch(bs[it % 2]), labs[it % 2])
        torch.cuda.synchronize()
        dt = (time.time() - t) / n
        print(f"{kind:14s}: {dt * 1e3:7.2f} ms per step = {B / dt:7.1f} pairs/s (eager launches, {B} pairs)", flush=True)


def decoder_batch(leg, b, B, T, seed):
    """the video keys of one batch of the leg; the pixels are random bytes (one random picture per source size, rolled per clip: the
    kernels' work does not depend on the values)"""
    import torch

    from tvts_amd.data_loader.transforms import resize_sizes
    from tvts_amd.data_loader.v2_input import failed_clip
    g = torch.Generator().manual_seed(seed)
    if leg == "fp32":
        return dict(video=b["video"].pin_memory())
    crops, clips = [], []
    base = {s: torch.randint(0, 256, (T,) + s + (3,), generator=g, dtype=torch.uint8) for s in SOURCES}
    for i in range(B):
        s = SOURCES[0] if leg == "u8_uniform" else SOURCES[i % 3]
        c = base[s].roll(i, 2)
        if leg == "u8_ragged_short" and i % 10 == 9:
            c, s = (c[:max(T // 2, 1)], s) if i % 20 == 9 else (failed_clip(IMG), (IMG, IMG))
        nh, nw = resize_sizes(s[0], s[1], SIZE)
        crops.append([int(torch.randint(0, nh - IMG + 1, (1,), generator=g)), int(torch.randint(0, nw - IMG + 1, (1,), generator=g))])
        clips.append(c.contiguous())
    out = dict(crop=torch.tensor(crops, dtype=torch.int32), resize=SIZE)
    if leg == "u8_uniform":
        out["video"] = torch.stack(clips).pin_memory()
    else:
        out.update(video=clips, num_frames=T)
    return out


def run_leg(leg, B, T, blocks, steps):
    import torch

    from tvts_amd import arch as A
    from tvts_amd import hip as K
    from tvts_amd.data_loader import synth_batch
    a = dict(A.ARCHS["B_16"])
    m, run = build(a)
    pool = []
    for i in range(2):
        b = synth_batch(a, B, T, seed=i, caption_len=32)
        b.update(decoder_batch(leg, b, B, T, 100 + i))
        pool.append(b)
    labels = [b["label"].reshape(-1).to(torch.int32).to("cuda:0") for b in pool]
    events, pack_ms = [], []
    name = {"u8_uniform": "patch_gather_u8", "fp32": "patch_gather"}.get(leg, "patch_gather_u8_ragged")
    inner = getattr(K, name)

    def timed(*args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        inner(*args, **kw)
        e1.record()
        events.append((e0, e1))
    setattr(K, name, timed)
    if leg.startswith("u8_ragged"):
        packed = m.engine._packed_to_device

        def timed_pack(clips, plan):
            t = time.perf_counter()
            out = packed(clips, plan)
            pack_ms.append((time.perf_counter() - t) * 1e3)
            return out
        m.engine._packed_to_device = timed_pack
    for it in range(3):
        run.run(m.engine.prepare_batch(pool[it % 2]), labels[it % 2])
    torch.cuda.synchronize()
    del events[:], pack_ms[:]
    ms = []
    for _ in range(blocks):
        t = time.perf_counter()
        for it in range(steps):
            run.run(m.engine.prepare_batch(pool[it % 2]), labels[it % 2])
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3 / steps)
    v = pool[0]["video"]
    nbytes = sum(c.numel() for c in v) if isinstance(v, list) else v.numel() * v.element_size()
    return dict(leg=leg, B=B, T=T, ms_per_step=ms, h2d_bytes=int(nbytes), gather=name,
                gather_ms=statistics.median(e0.elapsed_time(e1) for e0, e1 in events),
                pack_ms=statistics.median(pack_ms) if pack_ms else None)


def main():
    if len(sys.argv) <= 1 or not sys.argv[1].startswith("--"):
        one_process(int(sys.argv[1]) if len(sys.argv) > 1 else 192)
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", action="store_true")
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.leg:
        print("LEG " + json.dumps(run_leg(args.leg, args.batch, args.frames, args.blocks, args.steps)), flush=True)
        return
    res = {leg: dict(ms=[], h2d_bytes=None, gather=None, gather_ms=[], pack_ms=[]) for leg in LEGS}
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
            res[leg]["h2d_bytes"], res[leg]["gather"] = r["h2d_bytes"], r["gather"]
            res[leg]["gather_ms"].append(r["gather_ms"])
            if r["pack_ms"] is not None:
                res[leg]["pack_ms"].append(r["pack_ms"])
            print(f"round {rnd} {leg:15s} {['%.2f' % v for v in r['ms_per_step']]} ms/step, {r['gather']} {r['gather_ms']:.3f} ms"
                  + (f", host packing {r['pack_ms']:.1f} ms" if r["pack_ms"] is not None else ""), flush=True)
    base = statistics.median(res["fp32"]["ms"])
    summary = dict(batch=args.batch, frames=args.frames, legs={})
    for leg in LEGS:
        r = res[leg]
        med = statistics.median(r["ms"])
        summary["legs"][leg] = dict(median_ms=med, min_ms=min(r["ms"]), max_ms=max(r["ms"]), vs_fp32=med / base,
                                    pairs_per_s=args.batch / med * 1e3, h2d_MB=r["h2d_bytes"] / 1e6, gather=r["gather"],
                                    gather_ms=statistics.median(r["gather_ms"]),
                                    pack_ms=statistics.median(r["pack_ms"]) if r["pack_ms"] else None)
        print(f"{leg:15s} median {med:7.2f} ms/step ({min(r['ms']):.2f} .. {max(r['ms']):.2f})  x{med / base:.3f} of fp32  "
              f"{args.batch / med * 1e3:7.1f} pairs/s  H2D {r['h2d_bytes'] / 1e6:7.1f} MB  {r['gather']} {statistics.median(r['gather_ms']):.3f} ms"
              + (f"  host packing {statistics.median(r['pack_ms']):.1f} ms" if r["pack_ms"] else ""), flush=True)
    print("RESULT " + json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
