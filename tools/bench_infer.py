#!/usr/bin/env python3
"""The forward-only video encoder against the training-path forward (GPU dev tool): clips/s and peak allocated GB of
`compute_video` under no_grad (Engine.video_forward) and of `encode_video` (Engine.encode_video) at the downstream geometry
(12 unmasked frames), B/16 at 32 / 128 clips and H/14 at 8 / 32 clips; and the full-frame SPACE attention site alone, the
streaming kernel + CLS-query pair (what calls with lse2 run) against the forward-only fused kernel.  One JSON line each.
  --attn-only: the attention lines only (for a `rocprofv3 --kernel-trace --stats` run of its own).
  --mc: the SSv2 multiple-choice workload instead (174 candidate captions for each of 16 clips): encode_text(packed=False) against
  encode_text(packed=True), the packed attention site against the rectangular one, and the whole _mc forward; B/16 and H/14.
  The caption lengths are a STAND-IN (uniform in [6, 24] from a fixed seed): the SSv2 label files are not part of this repository.
  --fp8: H/14 `encode_video` on the e4m3 architecture (arch["fp8"]: the blocks' GEMMs on e4m3 copies, per-token activation scales)
  against the bf16 architecture, same random weights, at the H/14 clip counts above; one line per form.
  --v1: the v1 model (tubelet ViT-B/16, joint attention) at 16 full frames (S = 1569): `TVTS.encode_video` (fp32 and uint8 clips)
  against the eval-mode training forward `compute_video` under no_grad, clips/s and peak allocated GB at 4 / 16 clips."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

CONFIGS = [("B_16", 196, 32), ("B_16", 196, 128), ("H_14", 256, 8), ("H_14", 256, 32)]


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def attention(K):
    """one SPACE site of each geometry at 128 / 32 clips (B/16 heads 12 dh 64, H/14 heads 16 dh 80), T = 12"""
    for name, B, n, heads, dh in (("B_16", 128, 196, 12, 64), ("H_14", 32, 256, 16, 80)):
        T, W = 12, heads * dh
        S = 1 + T * n
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B * S, 3 * W, generator=g, device="cuda").bfloat16()
        out = torch.empty(B * S, W, dtype=torch.bfloat16, device="cuda")
        ws = torch.empty(B * heads * T * (dh + 2), device="cuda")
        res = {}
        for form, fused in (("streaming + CLS pass", False), ("fused full-frame", True)):
            res[form] = timed(lambda: K.attn_fwd_divided("space", qkv, out, None, ws, B=B, heads=heads, S=S, T=T, n=n,
                                                         head_dim=dh, fused=fused), 20)
        print(json.dumps({"what": f"SPACE attention forward-only, {name} T=12 n={n}", "clips": B,
                          **{k + " us": 1e6 * v for k, v in res.items()}}), flush=True)
        del qkv, out, ws
        torch.cuda.empty_cache()


def median_alternated(fns, reps, warmup=3):
    """{name: median seconds per call}, the calls alternated in one process, each timed with its own synchronisation"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


def multiple_choice(K, reps):
    import importlib
    from tvts_amd.model._common import pack_captions
    C, B, T, lo, hi = 174, 16, 12, 6, 24
    N = C * B
    lens = torch.randint(lo, hi + 1, (N,), generator=torch.Generator().manual_seed(0))
    note = f"caption lengths: stand-in, uniform in [{lo}, {hi}], seed 0 (the SSv2 label files are not available here)"
    rows_packed, rows_rect = int(lens.sum()), N * int(lens.max())
    for name, n in (("B_16", 196), ("H_14", 256)):
        mod = importlib.import_module(f"tvts_amd.downstream.model_TVTSv2_ViT_{name}_mc")
        m = getattr(mod, f"TVTSv2_{name}")(load_checkpoint=None, pretrained=False)
        a = m.arch
        g = torch.Generator().manual_seed(1)
        ids = torch.zeros(N, a["context"], dtype=torch.int64)
        ids[:, 0] = a["vocab"] - 2
        body = torch.randint(1, a["vocab"] - 408, (N, a["context"]), generator=g)
        col = torch.arange(a["context"]).unsqueeze(0)
        inside = (col >= 1) & (col < (lens - 1).unsqueeze(1))
        ids[inside] = body[inside]
        ids[torch.arange(N), lens - 1] = a["vocab"] - 1
        with torch.no_grad():
            med = median_alternated({"rectangular": lambda: m.encode_text(ids), "packed": lambda: m.encode_text(ids, packed=True)}, reps)
        t0 = time.perf_counter()
        for _ in range(reps):
            pack_captions(ids, ids.argmax(-1))
        host = (time.perf_counter() - t0) / reps
        print(json.dumps({"what": f"encode_text, {name}, {N} captions", "note": note, "token rows packed": rows_packed,
                          "token rows rectangular": rows_rect, "row ratio": rows_packed / rows_rect, "reps": reps,
                          "rectangular ms (median)": 1e3 * med["rectangular"], "packed ms (median, host packing included)": 1e3 * med["packed"],
                          "host packing ms (mean, inside the packed figure)": 1e3 * host,
                          "packed / rectangular": med["packed"] / med["rectangular"]}), flush=True)
        # the attention site alone, on the same captions
        heads, L = a["text_heads"], int(lens.max())
        W = heads * 64
        _, seq_start, _, max_len = pack_captions(ids, ids.argmax(-1))
        seq_start = seq_start.cuda()
        gd = torch.Generator(device="cuda").manual_seed(2)
        qp = torch.randn(rows_packed, 3 * W, generator=gd, device="cuda").bfloat16()
        qr = torch.randn(rows_rect, 3 * W, generator=gd, device="cuda").bfloat16()
        op, orr = torch.empty(rows_packed, W, dtype=torch.bfloat16, device="cuda"), torch.empty(rows_rect, W, dtype=torch.bfloat16, device="cuda")
        med = median_alternated({"rectangular": lambda: K.attn_fwd("full", qr, orr, None, B=N, heads=heads, S=L, causal=True),
                                 "packed": lambda: K.attn_fwd_packed(qp, seq_start, op, N=N, heads=heads, max_len=max_len)}, reps)
        print(json.dumps({"what": f"text attention site, {name}, {N} captions, {heads} heads", "note": note,
                          "rectangular S=%d us (median, launch + sync)" % L: 1e6 * med["rectangular"],
                          "packed us (median, launch + sync)": 1e6 * med["packed"]}), flush=True)
        del qp, qr, op, orr
        # the whole multiple-choice forward
        v = torch.randn(B, T, 3, 224, 224, generator=g).cuda()
        data = {"text": ids, "video": v, "keep_ind": torch.arange(n).unsqueeze(0)}
        m.engine._inf.clear()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        dt = median_alternated({"mc": lambda: m(data)}, max(reps // 4, 5), warmup=2)["mc"]
        print(json.dumps({"what": f"multiple-choice forward, {name}, B={B} T={T} C={C}", "note": note, "clips/s": B / dt,
                          "ms": 1e3 * dt, "peak GB": torch.cuda.max_memory_allocated() / 1e9}), flush=True)
        del m, v, data
        torch.cuda.empty_cache()


def fp8_encoders(iters):
    """H/14 encode_video, bf16 against e4m3 (one model alive at a time); the e4m3 line also carries the worst per-clip cosine of
    its embeddings against the bf16 model's"""
    from tvts_amd.arch import ARCHS
    from tvts_amd.downstream.model_TVTSv2_ViT_H_14 import TVTSv2_H_14
    name, n = "H_14", 256
    keep = torch.arange(n).unsqueeze(0)
    ref = {}
    for form, over in (("bf16", {}), ("e4m3", {"fp8": True})):
        m = TVTSv2_H_14(load_checkpoint=None, arch=dict(ARCHS[name], **over), pretrained=False)
        for cfg, _, B in CONFIGS:
            if cfg != name:
                continue
            v = torch.randn(B, 12, 3, 224, 224, generator=torch.Generator().manual_seed(1)).cuda()
            m.engine._inf.clear()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            dt = timed(lambda: m.encode_video(v, keep), iters)
            line = {"what": f"encode_video, {name} T=12 n={n}, {form}", "clips": B, "clips/s": B / dt,
                    "peak GB": torch.cuda.max_memory_allocated() / 1e9}
            e = m.encode_video(v, keep).double().cpu()
            if form == "bf16":
                ref[B] = e
            else:
                line["worst cosine against bf16"] = float(torch.nn.functional.cosine_similarity(e, ref[B], dim=1).min())
            print(json.dumps(line), flush=True)
            del v
        del m
        torch.cuda.empty_cache()


def v1_encoders(iters):
    """the v1 model with random weights (a one-layer text tower: it takes no part), 16 frames, every patch of every tube"""
    import types
    from tvts_amd.arch import ARCH_V1
    from tvts_amd.model.model_dist_TVTS import TVTS
    m = TVTS(types.SimpleNamespace(local_rank=0, rank=0, world_size=1), arch=dict(ARCH_V1, text_layers=1, sort_depth=1)).eval()
    T, ppf = 16, 196
    eng = m.engine
    for B in (4, 16):
        g = torch.Generator().manual_seed(1)
        v = torch.randn(B, T, 3, 224, 224, generator=g).cuda()
        u8 = torch.randint(0, 256, (B, T, 224, 224, 3), generator=g, dtype=torch.uint8).cuda()
        keep = torch.arange(ppf).view(1, 1, ppf).expand(B, T // 2, ppf)
        line = {"what": f"video embeddings, v1 T={T} S={1 + T // 2 * ppf}", "clips": B}
        for form, fn in (("training forward (eval mode)", lambda: m.compute_video(v, keep)),
                         ("encode_video", lambda: m.encode_video(v)), ("encode_video uint8", lambda: m.encode_video(u8))):
            eng.buf.clear(); eng._back.clear(); eng._seen.clear(); eng._inf.clear()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            try:
                with torch.no_grad():
                    dt = timed(fn, iters)
                line[form + " clips/s"] = B / dt
                line[form + " peak GB"] = torch.cuda.max_memory_allocated() / 1e9
            except torch.cuda.OutOfMemoryError:
                line[form + " clips/s"] = None
                line[form + " peak GB"] = "out of memory"
        print(json.dumps(line), flush=True)
        del v, u8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attn-only", action="store_true")
    ap.add_argument("--mc", action="store_true")
    ap.add_argument("--fp8", action="store_true")
    ap.add_argument("--v1", action="store_true")
    ap.add_argument("--reps", type=int, default=20, help="--mc: timed repetitions of each form (median)")
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    from tvts_amd import hip as K
    if args.mc:
        multiple_choice(K, max(args.reps, 20))
        return
    if args.fp8:
        fp8_encoders(args.iters)
        return
    if args.v1:
        v1_encoders(args.iters)
        return
    attention(K)
    if args.attn_only:
        return
    import importlib
    models = {}
    for name, n, B in CONFIGS:
        m = models.get(name)
        if m is None:
            for k in list(models):
                del models[k]
            torch.cuda.empty_cache()
            mod = importlib.import_module(f"tvts_amd.downstream.model_TVTSv2_ViT_{name}")
            m = models[name] = getattr(mod, f"TVTSv2_{name}")(load_checkpoint=None, pretrained=False)
        g = torch.Generator().manual_seed(1)
        v = torch.randn(B, 12, 3, 224, 224, generator=g).cuda()
        keep = torch.arange(n).unsqueeze(0)
        line = {"what": f"video embeddings, {name} T=12 n={n}", "clips": B}
        for form, fn in (("training forward", lambda: m.compute_video(v, keep.expand(B, -1))),
                         ("encode_video", lambda: m.encode_video(v, keep))):
            eng = m.engine
            eng.buf.clear(); eng._back.clear(); eng._seen.clear(); eng._inf.clear()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            try:
                with torch.no_grad():
                    dt = timed(fn, args.iters)
                line[form + " clips/s"] = B / dt
                line[form + " peak GB"] = torch.cuda.max_memory_allocated() / 1e9
            except torch.cuda.OutOfMemoryError:
                line[form + " clips/s"] = None
                line[form + " peak GB"] = "out of memory"
        print(json.dumps(line), flush=True)
        del v


if __name__ == "__main__":
    main()
